// pybind.cpp -- Python view of the C++ host layer, used by tests/test_host_layer.py so that the parity tests
// drive ICP::align() exactly the way mola::LidarOdometry does (LidarOdometry.cpp:961-962).
#include <cstring>
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "mola_lidar_odometry_hip/LidarOdometry.h"
#include "mola_lidar_odometry_hip/LoopClosure.h"
#include "mola_lidar_odometry_hip/MapCleaning.h"
#include "mola_lidar_odometry_hip/OccupancyGrid.h"
#include "mola_lidar_odometry_hip/Traversability.h"
#include "mola_lidar_odometry_hip/NavCostmap.h"
#include "mola_lidar_odometry_hip/Replan.h"
#include "mola_lidar_odometry_hip/RoutePlan.h"
#include "mola_lidar_odometry_hip/SessionJoin.h"
#include "mp2p_icp_hip/mp2p_icp_hip.h"
#include "molahip_host/plugin_switches.h"

namespace py = pybind11;
using namespace mp2p_icp_hip;

static std::shared_ptr<PointCloud> make_cloud(py::array_t<float, py::array::c_style | py::array::forcecast> xyz) {
  auto c = std::make_shared<PointCloud>();
  auto r = xyz.unchecked<2>();
  for (py::ssize_t i = 0; i < r.shape(0); i++) c->insertPoint(r(i, 0), r(i, 1), r(i, 2));
  return c;
}

PYBIND11_MODULE(_mp2p_icp_hip, m) {
  m.doc() = "mp2p_icp_hip: C++ host layer of libmolahip (mirrors the mp2p_icp plugin API)";
  py::class_<TPose3D>(m, "TPose3D")
      .def(py::init<>())
      .def(py::init([](double x, double y, double z, double yaw, double pitch, double roll) { return TPose3D{x, y, z, yaw, pitch, roll}; }))
      .def_readwrite("x", &TPose3D::x).def_readwrite("y", &TPose3D::y).def_readwrite("z", &TPose3D::z)
      .def_readwrite("yaw", &TPose3D::yaw).def_readwrite("pitch", &TPose3D::pitch).def_readwrite("roll", &TPose3D::roll);
  py::class_<CPose3D>(m, "CPose3D")
      .def(py::init<>())
      .def(py::init<const TPose3D&>())
      .def_static("from_matrix", [](std::vector<double> T) { CPose3D p; if (T.size() != 12) throw std::runtime_error("need 12 values"); std::copy(T.begin(), T.end(), p.T); return p; })
      .def("asTPose", &CPose3D::asTPose)
      .def("matrix", [](const CPose3D& p) { return std::vector<double>(p.T, p.T + 12); })
      .def("__add__", &CPose3D::operator+)
      .def("__sub__", &CPose3D::operator-);
  py::class_<CPose3DPDFGaussianInf>(m, "CPose3DPDFGaussianInf")
      .def(py::init([](const CPose3D& mean, std::vector<double> info) {
        CPose3DPDFGaussianInf p; p.mean = mean; if (info.size() != 36) throw std::runtime_error("need 36 values");
        std::copy(info.begin(), info.end(), p.cov_inv); return p; }));
  py::class_<Config>(m, "Config")
      .def_static("FromYamlText", &Config::FromYamlText)
      .def_static("FromYamlFile", &Config::FromYamlFile)
      .def("has", &Config::has)
      .def("__getitem__", [](const Config& c, const std::string& k) { return c[k]; })
      .def("at", [](const Config& c, size_t i) { return c.at(i); })
      .def("size", &Config::size)
      .def("asString", &Config::asString);
  m.def("evaluate_expression", &evaluate_expression);
  // MOLA_HIP_* switches (molahip_host/plugin_switches.h, shared with the mp2p_icp adapter): re-read the environment, and
  // show what was read -- what the adapter would pass to the C ABI for an upstream `RobustKernel::<name>`
  m.def("reload_plugin_switches", [] {
    molahip_host::reload_plugin_switches();   // this module's copy of the cache (what plugin_switches() below shows) ...
    mp2p_icp_hip::reload_plugin_switches();   // ... and the host library's, which is the one the alignments read
  });
  m.def("library_matched_points", [] { return mp2p_icp_hip::plugin_switch_matched_points(); });
  m.def("plugin_switches", [] {
    const auto& s = molahip_host::plugin_switches();
    py::dict d;
    d["gm_form"] = s.gm_form; d["index_mode"] = s.index_mode; d["cov_step_xyz"] = s.cov_step_xyz; d["cov_step_ang"] = s.cov_step_ang;
    d["min_delta"] = s.min_delta; d["max_cost"] = s.max_cost; d["pt2pl_mode"] = s.pt2pl_mode; d["matched_points"] = s.matched_points;
    d["far_voxel_metric"] = s.far_voxel_metric; d["force_cpu"] = s.force_cpu;
    return d;
  });
  m.def("plugin_switch_fuse_kbest", [] { return molahip_host::plugin_switches().fuse_kbest; });  // MOLA_HIP_FUSE_KBEST: -1 not set
  m.def("plugin_switch_fuse_planes", [] { return molahip_host::plugin_switches().fuse_planes; });  // MOLA_HIP_FUSE_PLANES: -1 not set
  m.def("plugin_switch_voxelmap_update", [] { return molahip_host::plugin_switches().voxelmap_update; });  // MOLA_HIP_VOXELMAP_UPDATE: MH_OCC_*
  m.def("plugin_switch_fuse_gates", [] { return molahip_host::plugin_switches().fuse_gates; });  // MOLA_HIP_FUSE_GATES: -1 not set (a function of its own: the keys of plugin_switches() are compared as a whole by their users)
  m.def("kernel_from_upstream_name", [](const std::string& n) { return molahip_host::kernel_from_upstream_name(n.c_str(), molahip_host::plugin_switches()); });
  m.def("term_reason_name", [](uint32_t t) { return std::string(enum2str(molahip_host::term_reason_to<IterTermReason>(t))); });
  m.def("evaluate_compiled", [](const std::string& e, const std::map<std::string, double>& v) { return CompiledExpression(e).evaluate(v); });
  py::class_<ParameterSource>(m, "ParameterSource")
      .def(py::init<>())
      .def("updateVariable", &ParameterSource::updateVariable)
      .def("realize", &ParameterSource::realize);
  py::class_<Layer, std::shared_ptr<Layer>>(m, "Layer");
  py::class_<PointCloud, Layer, std::shared_ptr<PointCloud>>(m, "PointCloud")
      .def(py::init(&make_cloud))
      .def("size", &PointCloud::size);
  py::class_<HashedVoxelPointCloud, Layer, std::shared_ptr<HashedVoxelPointCloud>>(m, "HashedVoxelPointCloud")
      .def(py::init([](float vs, uint32_t cap) { return std::make_shared<HashedVoxelPointCloud>(vs, cap); }))
      .def("setPoints", [](HashedVoxelPointCloud& h, py::array_t<float, py::array::c_style | py::array::forcecast> xyz) {
        auto c = make_cloud(xyz); h.setPoints(c->x.data(), c->y.data(), c->z.data(), c->size()); })
      .def("insertPoints", [](HashedVoxelPointCloud& h, py::array_t<float, py::array::c_style | py::array::forcecast> xyz) {
        auto c = make_cloud(xyz); h.insertPoints(c->x.data(), c->y.data(), c->z.data(), c->size()); })
      // frames: a sequence of (xyz [n, 3], T: 12 values); bit for bit what insertPointCloud(frame, T, 0) per frame gives
      .def("insertFrames", [](HashedVoxelPointCloud& h, const std::vector<std::pair<py::array_t<float, py::array::c_style | py::array::forcecast>, std::vector<double>>>& frames,
                              uint64_t max_points_per_pass) {
        std::vector<std::shared_ptr<PointCloud>> clouds;
        std::vector<PosedFrame> f;
        for (const auto& [xyz, T] : frames) {
          if (T.size() != 12) throw std::runtime_error("need 12 values");
          clouds.push_back(make_cloud(xyz));
          PosedFrame pf;
          pf.x = clouds.back()->x.data(); pf.y = clouds.back()->y.data(); pf.z = clouds.back()->z.data();
          pf.n = clouds.back()->size();
          std::copy(T.begin(), T.end(), pf.pose.T);
          f.push_back(pf);
        }
        h.insertFrames(f, max_points_per_pass); }, py::arg("frames"), py::arg("max_points_per_pass") = 0)
      .def("size", &HashedVoxelPointCloud::size)
      .def("voxelCount", &HashedVoxelPointCloud::voxelCount)
      .def("className", [](const HashedVoxelPointCloud& h) { return std::string(h.className()); })
      .def("saveToFile", &HashedVoxelPointCloud::saveToFile, py::arg("path"), py::arg("name") = "map", py::arg("remove_voxels_farther_than") = 0.f)
      .def("loadFromFile", &HashedVoxelPointCloud::loadFromFile, py::arg("path"), py::arg("name") = "")
      // (offsets, global_idx, xyz [k, 3], d2) of mh_nn_search_radius; T: 12 values, row-major [R|t]
      .def("radiusSearch", [](const HashedVoxelPointCloud& h, py::array_t<float, py::array::c_style | py::array::forcecast> xyz,
                              std::vector<double> T, double radius, bool sorted) {
        if (T.size() != 12) throw std::runtime_error("need 12 values");
        CPose3D P; std::copy(T.begin(), T.end(), P.T);
        auto c = make_cloud(xyz);
        const RadiusResults r = h.radiusSearch(c->x.data(), c->y.data(), c->z.data(), c->size(), P, radius, sorted);
        const py::ssize_t k = (py::ssize_t)r.globalIdx.size();
        py::array_t<float> pts({k, (py::ssize_t)3});
        auto w = pts.mutable_unchecked<2>();
        for (py::ssize_t i = 0; i < k; i++) { w(i, 0) = r.gx[i]; w(i, 1) = r.gy[i]; w(i, 2) = r.gz[i]; }
        return py::make_tuple(py::array_t<uint32_t>((py::ssize_t)r.offsets.size(), r.offsets.data()),
                              py::array_t<uint32_t>(k, r.globalIdx.data()), pts, py::array_t<float>(k, r.errSq.data()));
      }, py::arg("queries"), py::arg("T"), py::arg("radius"), py::arg("sorted") = false);
  py::class_<SparseTreesPointCloud, HashedVoxelPointCloud, std::shared_ptr<SparseTreesPointCloud>>(m, "SparseTreesPointCloud")
      .def(py::init([](float grid, float clearance) { return std::make_shared<SparseTreesPointCloud>(grid, clearance); }));
  py::class_<CVoxelMap, HashedVoxelPointCloud, std::shared_ptr<CVoxelMap>>(m, "CVoxelMap")
      .def(py::init([](float resolution) { return std::make_shared<CVoxelMap>(CVoxelMap::defaultParams(resolution)); }))
      .def("insertPointCloud", [](CVoxelMap& v, py::array_t<float, py::array::c_style | py::array::forcecast> xyz, std::vector<double> T,
                                  float remove_voxels_farther_than) {
        if (T.size() != 12) throw std::runtime_error("need 12 values");
        CPose3D P; std::copy(T.begin(), T.end(), P.T);
        auto c = make_cloud(xyz);
        DevicePointCloud pc(v.context());
        pc.setPoints(c->x.data(), c->y.data(), c->z.data(), c->size());
        v.insertPointCloud(pc, P, remove_voxels_farther_than);
      }, py::arg("xyz"), py::arg("T"), py::arg("remove_voxels_farther_than") = 0.f)
      .def("searchVoxelSize", &CVoxelMap::searchVoxelSize)
      // frames: a list of (xyz [n, 3], T [12]) ray-traced at once (mh_occmap_insert_frames)
      .def("insertPointCloudFrames", [](CVoxelMap& v, const std::vector<std::pair<py::array_t<float, py::array::c_style | py::array::forcecast>, std::vector<double>>>& frames,
                                        uint64_t max_points_per_pass) {
        std::vector<decltype(make_cloud(frames[0].first))> clouds;
        std::vector<PosedFrame> f;
        for (const auto& [xyz, T] : frames) {
          if (T.size() != 12) throw std::runtime_error("need 12 values");
          clouds.push_back(make_cloud(xyz));
          PosedFrame pf;
          pf.x = clouds.back()->x.data(); pf.y = clouds.back()->y.data(); pf.z = clouds.back()->z.data();
          pf.n = clouds.back()->size();
          std::copy(T.begin(), T.end(), pf.pose.T);
          f.push_back(pf);
        }
        v.insertPointCloudFrames(f, max_points_per_pass); }, py::arg("frames"), py::arg("max_points_per_pass") = 0)
      // (lo [3], hi [3]) of the stored cells' indices, or None for an empty map
      .def("indexBounds", [](const CVoxelMap& v) -> py::object {
        int32_t lo[3], hi[3];
        if (!v.indexBounds(lo, hi)) return py::none();
        return py::make_tuple(py::make_tuple(lo[0], lo[1], lo[2]), py::make_tuple(hi[0], hi[1], hi[2])); })
      // int32 [ny, nx]: the maximum log-odds per column of the band z_lo..z_hi (cell indices), INT32_MIN where nothing is stored
      .def("projectGrid", [](const CVoxelMap& v, int32_t x0, int32_t y0, uint32_t nx, uint32_t ny, int32_t z_lo, int32_t z_hi) {
        mh_occgrid_window w{};
        w.x0 = x0; w.y0 = y0; w.nx = nx; w.ny = ny; w.z_lo = z_lo; w.z_hi = z_hi;
        const std::vector<int32_t> g = v.projectGrid(w);
        py::array_t<int32_t> out({(py::ssize_t)ny, (py::ssize_t)nx});
        std::copy(g.begin(), g.end(), out.mutable_data());
        return out; }, py::arg("x0"), py::arg("y0"), py::arg("nx"), py::arg("ny"), py::arg("z_lo"), py::arg("z_hi"))
      // (keys int32 [n, 3], log-odds int32 [n]) in ascending key order
      .def("download", [](const CVoxelMap& v) {
        std::vector<int32_t> k, l;
        v.download(k, l);
        py::array_t<int32_t> keys({(py::ssize_t)l.size(), (py::ssize_t)3});
        std::copy(k.begin(), k.end(), keys.mutable_data());
        return py::make_tuple(keys, py::array_t<int32_t>((py::ssize_t)l.size(), l.data())); });
  py::class_<NDT, HashedVoxelPointCloud, std::shared_ptr<NDT>>(m, "NDT")
      .def(py::init([](float vs, uint32_t cap, float min_dist, float ratio) { return std::make_shared<NDT>(vs, cap, min_dist, ratio); }))
      .def("planeCount", &NDT::planeCount);
  py::class_<metric_map_t>(m, "metric_map_t")
      .def(py::init<>())
      .def("set_layer", [](metric_map_t& mm, const std::string& n, std::shared_ptr<Layer> l) { mm.layers[n] = std::move(l); });
  py::class_<Parameters>(m, "Parameters")
      .def(py::init<>())
      .def_readwrite("maxIterations", &Parameters::maxIterations)
      .def_readwrite("minAbsStep_trans", &Parameters::minAbsStep_trans)
      .def_readwrite("minAbsStep_rot", &Parameters::minAbsStep_rot)
      .def_readwrite("generateDebugFiles", &Parameters::generateDebugFiles)
      .def_readwrite("debugFileNameFormat", &Parameters::debugFileNameFormat);
  py::enum_<IterTermReason>(m, "IterTermReason")
      .value("Undefined", IterTermReason::Undefined).value("NoPairings", IterTermReason::NoPairings)
      .value("SolverError", IterTermReason::SolverError).value("MaxIterations", IterTermReason::MaxIterations)
      .value("Stalled", IterTermReason::Stalled).value("QualityCheckpointFailed", IterTermReason::QualityCheckpointFailed)
      .value("HookRequest", IterTermReason::HookRequest);
  py::class_<Results>(m, "Results")
      .def(py::init<>())
      .def_readonly("quality", &Results::quality)
      .def_readonly("nIterations", &Results::nIterations)
      .def_readonly("terminationReason", &Results::terminationReason)
      .def("pose", [](const Results& r) { return std::vector<double>(r.optimal_tf.mean.T, r.optimal_tf.mean.T + 12); })
      .def("cov", [](const Results& r) { return std::vector<double>(r.optimal_tf.cov, r.optimal_tf.cov + 36); })
      .def("n_pairs", [](const Results& r) { return r.finalPairings.size(); })
      .def("n_pairs_pt2pl", [](const Results& r) { return r.finalPairings.pl_lx.size(); })
      .def("potential_pairings", [](const Results& r) { return r.finalPairings.potential_pairings; })
      .def("pair_global_idx", [](const Results& r) { return r.finalPairings.globalIdx; })
      .def("pair_local_idx", [](const Results& r) { return r.finalPairings.localIdx; })
      // the point-to-plane pairings, nine values each: local point | plane centroid | plane normal
      .def("pairs_pt2pl", [](const Results& r) {
        const Pairings& f = r.finalPairings;
        std::vector<std::vector<float>> out(f.pl_lx.size());
        for (size_t k = 0; k < out.size(); k++)
          out[k] = {f.pl_lx[k], f.pl_ly[k], f.pl_lz[k], f.pl_cx[k], f.pl_cy[k], f.pl_cz[k], f.pl_nx[k], f.pl_ny[k], f.pl_nz[k]};
        return out;
      });
  py::class_<ICP, std::shared_ptr<ICP>>(m, "ICP")
      .def("align", [](ICP& icp, const metric_map_t& l, const metric_map_t& g, const TPose3D& guess, const Parameters& p,
                       std::optional<CPose3DPDFGaussianInf> prior) { Results r; icp.align(l, g, guess, p, r, prior); return r; },
           py::arg("pcLocal"), py::arg("pcGlobal"), py::arg("initialGuess"), py::arg("params"), py::arg("prior") = std::nullopt)
      .def("attachToParameterSource", &ICP::attachToParameterSource)
      .def("setDeviceHook", &ICP::setDeviceHook)
      .def("clearHooks", &ICP::clearHooks)
      .def("forceGenericPath", &ICP::forceGenericPath)
      .def("fuseGatedMatchers", &ICP::fuseGatedMatchers)
      .def("fuseMultiPairings", &ICP::fuseMultiPairings)
      .def("fusePlaneMatchers", &ICP::fusePlaneMatchers)
      .def("alignPath", &ICP::alignPath)
      .def("precomputeSchedule", &ICP::precomputeSchedule)
      .def("setHookReplay", &ICP::setHookReplay)
      .def("setKeepFinalPairings", &ICP::setKeepFinalPairings)
      .def("lastAlignUsedFusedPath", &ICP::lastAlignUsedFusedPath)
      .def("setIterationHook", [](ICP& icp, std::function<bool(uint32_t, std::vector<double>)> f) {
        icp.setIterationHook([f](const ICP::IterationHook_Input& in) {
          ICP::IterationHook_Output o;
          o.request_stop = f(in.currentIteration, std::vector<double>(in.currentSolution->optimalPose.T, in.currentSolution->optimalPose.T + 12));
          return o; }); });
  // ---- key-frames (molahip_host/keyframe_file.h) as dicts: {"maps": [{name, class_name, params, remove_voxels_farther_than}],
  // "frames": [{timestamp, pose [12], cov [36], twist [6] or None, layers: None (a frame without points) or [(map_index, xyz [n, 3])]}]}
  auto params2dict = [](const mh_map_params& q) {
    py::dict p;
    p["voxel_size"] = q.voxel_size; p["max_points_per_voxel"] = q.max_points_per_voxel; p["index_mode"] = q.index_mode;
    p["min_distance_between_points"] = q.min_distance_between_points; p["ndt_max_eigen_ratio"] = q.ndt_max_eigen_ratio;
    p["ndt_min_points"] = q.ndt_min_points; p["far_voxel_metric"] = q.far_voxel_metric;
    return p;
  };
  auto dict2params = [](const py::dict& p) {
    mh_map_params q{};
    q.voxel_size = p["voxel_size"].cast<float>();
    q.max_points_per_voxel = p["max_points_per_voxel"].cast<uint32_t>();
    q.index_mode = p["index_mode"].cast<uint32_t>();
    q.min_distance_between_points = p["min_distance_between_points"].cast<float>();
    q.ndt_max_eigen_ratio = p["ndt_max_eigen_ratio"].cast<float>();
    q.ndt_min_points = p["ndt_min_points"].cast<uint32_t>();
    q.far_voxel_metric = p["far_voxel_metric"].cast<uint32_t>();
    return q;
  };
  auto kfset2dict = [params2dict](const molahip_host::KeyFrameSet& set) {
    py::list maps, frames;
    for (const auto& t : set.maps) {
      py::dict d;
      d["name"] = t.name; d["class_name"] = t.class_name; d["params"] = params2dict(t.params);
      d["remove_voxels_farther_than"] = t.remove_voxels_farther_than;
      maps.append(d);
    }
    for (const auto& f : set.frames) {
      py::dict d;
      d["timestamp"] = f.timestamp;
      d["pose"] = std::vector<double>(f.pose, f.pose + 12);
      d["cov"] = std::vector<double>(f.cov, f.cov + 36);
      d["twist"] = f.has_twist ? py::object(py::cast(std::vector<double>(f.twist, f.twist + 6))) : py::object(py::none());
      if (f.has_points) {
        py::list layers;
        for (const auto& l : f.layers) {
          const py::ssize_t n = (py::ssize_t)l.x.size();
          py::array_t<float> xyz({n, (py::ssize_t)3});
          auto w = xyz.mutable_unchecked<2>();
          for (py::ssize_t i = 0; i < n; i++) { w(i, 0) = l.x[i]; w(i, 1) = l.y[i]; w(i, 2) = l.z[i]; }
          layers.append(py::make_tuple(l.map_index, xyz));
        }
        d["layers"] = layers;
      } else {
        d["layers"] = py::none();
      }
      frames.append(d);
    }
    py::dict out;
    out["maps"] = maps; out["frames"] = frames;
    return out;
  };
  auto dict2kfset = [dict2params](const py::dict& in) {
    molahip_host::KeyFrameSet set;
    for (const py::handle& h : in["maps"].cast<py::list>()) {
      const py::dict d = h.cast<py::dict>();
      molahip_host::KeyFrameTarget t;
      t.name = d["name"].cast<std::string>();
      t.class_name = d["class_name"].cast<std::string>();
      t.params = dict2params(d["params"].cast<py::dict>());
      t.remove_voxels_farther_than = d["remove_voxels_farther_than"].cast<float>();
      set.maps.push_back(std::move(t));
    }
    for (const py::handle& h : in["frames"].cast<py::list>()) {
      const py::dict d = h.cast<py::dict>();
      molahip_host::KeyFrame f;
      f.timestamp = d["timestamp"].cast<double>();
      const auto pose = d["pose"].cast<std::vector<double>>();
      const auto cov = d["cov"].cast<std::vector<double>>();
      if (pose.size() != 12 || cov.size() != 36) throw std::runtime_error("a frame needs 12 pose values and 36 covariance values");
      std::copy(pose.begin(), pose.end(), f.pose);
      std::copy(cov.begin(), cov.end(), f.cov);
      if (!d["twist"].is_none()) {
        const auto tw = d["twist"].cast<std::vector<double>>();
        if (tw.size() != 6) throw std::runtime_error("a twist has 6 values");
        f.has_twist = true;
        std::copy(tw.begin(), tw.end(), f.twist);
      }
      if (!d["layers"].is_none()) {
        f.has_points = true;
        for (const py::handle& lh : d["layers"].cast<py::list>()) {
          const py::tuple lt = lh.cast<py::tuple>();
          molahip_host::KeyFrameLayer l;
          l.map_index = lt[0].cast<uint32_t>();
          auto xyz = lt[1].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
          if (xyz.ndim() != 2 || xyz.shape(1) != 3) throw std::runtime_error("a layer's xyz must be [n, 3]");
          const py::ssize_t n = xyz.shape(0);
          auto a = xyz.unchecked<2>();
          l.x.resize(n); l.y.resize(n); l.z.resize(n);
          for (py::ssize_t i = 0; i < n; i++) { l.x[i] = a(i, 0); l.y[i] = a(i, 1); l.z[i] = a(i, 2); }
          f.layers.push_back(std::move(l));
        }
      }
      set.frames.push_back(std::move(f));
    }
    return set;
  };
  m.def("write_keyframe_file", [dict2kfset](const std::string& path, const py::dict& set) { molahip_host::write_keyframe_file(path, dict2kfset(set)); });
  m.def("read_keyframe_file", [kfset2dict](const std::string& path) { return kfset2dict(molahip_host::read_keyframe_file(path)); });
  m.attr("KEYFRAME_FILE_VERSION") = molahip_host::kKeyFrameFileVersion;
  auto maps2list = [params2dict](const std::vector<molahip_host::LocalMapRecord>& recs) {
    py::list out;
    for (const auto& r : recs) {
      py::dict d;
      d["name"] = r.name; d["class_name"] = r.class_name; d["params"] = params2dict(r.params);
      d["remove_voxels_farther_than"] = r.remove_voxels_farther_than; d["n_offered"] = r.n_offered;
      const py::ssize_t n = (py::ssize_t)r.x.size();
      py::array_t<float> xyz({n, (py::ssize_t)3});
      auto w = xyz.mutable_unchecked<2>();
      for (py::ssize_t i = 0; i < n; i++) { w(i, 0) = r.x[i]; w(i, 1) = r.y[i]; w(i, 2) = r.z[i]; }
      d["xyz"] = xyz;
      d["src_idx"] = py::array_t<uint32_t>(n, r.src_idx.data());
      out.append(d);
    }
    return out;
  };
  // the maps of the whole drive from key-frames (a dict as above, or the path of a key-frame file): a list of map dicts as
  // read_local_map_file returns them; with `local_map_file` they are also written there (a version-1 local-map file)
  m.def("build_session_maps", [dict2kfset, maps2list](const py::object& frames, uint64_t max_points_per_pass, const std::string& local_map_file) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    std::vector<molahip_host::LocalMapRecord> recs;
    {
      py::gil_scoped_release nogil;
      recs = mola_hip::build_session_maps(set, nullptr, max_points_per_pass);
      if (!local_map_file.empty()) molahip_host::write_local_map_file(local_map_file, recs);
    }
    return maps2list(recs); }, py::arg("frames"), py::arg("max_points_per_pass") = 0, py::arg("local_map_file") = "");
  // place recognition over key-frames (mola_hip::PlaceIndex): the descriptor parameters as keywords, key-frame sets as the dicts above
  auto place_params = [](uint32_t rings, uint32_t sectors, float min_range, float max_range, float z_min, float z_max) {
    mh_place_params p{};
    p.n_rings = rings; p.n_sectors = sectors; p.min_range = min_range; p.max_range = max_range; p.z_min = z_min; p.z_max = z_max;
    return p;
  };
  auto desc2array = [](const std::vector<uint8_t>& d, const mh_place_params& p) {
    py::array_t<uint8_t> a({(py::ssize_t)p.n_rings, (py::ssize_t)p.n_sectors});
    std::copy(d.begin(), d.end(), a.mutable_data());
    return a;
  };
  py::class_<mola_hip::PlaceIndex>(m, "PlaceIndex")
      .def(py::init([place_params](uint32_t rings, uint32_t sectors, float min_range, float max_range, float z_min, float z_max) {
             return std::make_unique<mola_hip::PlaceIndex>(place_params(rings, sectors, min_range, max_range, z_min, z_max)); }),
           py::arg("n_rings") = 20, py::arg("n_sectors") = 64, py::arg("min_range") = 1.0f, py::arg("max_range") = 80.0f,
           py::arg("z_min") = -3.0f, py::arg("z_max") = 27.0f)
      .def("add_keyframes", [dict2kfset](mola_hip::PlaceIndex& ix, const py::object& frames, size_t first) {
        const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                             : dict2kfset(frames.cast<py::dict>());
        return ix.addKeyFrames(set, first); }, py::arg("frames"), py::arg("first") = 0)
      // [(frame, shift, dist)] ranked by (dist ascending, frame ascending)
      .def("query", [](const mola_hip::PlaceIndex& ix, py::array_t<float, py::array::c_style | py::array::forcecast> xyz) {
        auto c = make_cloud(xyz);
        DevicePointCloud d(DeviceContext::Default());
        d.setPoints(c->x.data(), c->y.data(), c->z.data(), c->size());
        py::list out;
        for (const auto& k : ix.query(d)) out.append(py::make_tuple(k.frame, k.shift, k.dist));
        return out; })
      .def("size", &mola_hip::PlaceIndex::size);
  // the descriptor of one layer (xyz [n, 3], vehicle frame): uint8 [n_rings, n_sectors]
  m.def("place_describe", [place_params, desc2array](py::array_t<float, py::array::c_style | py::array::forcecast> xyz, uint32_t rings, uint32_t sectors,
                                                     float min_range, float max_range, float z_min, float z_max) {
    const mh_place_params p = place_params(rings, sectors, min_range, max_range, z_min, z_max);
    auto c = make_cloud(xyz);
    DevicePointCloud d(DeviceContext::Default());
    d.setPoints(c->x.data(), c->y.data(), c->z.data(), c->size());
    std::vector<uint8_t> desc((size_t)rings * sectors);
    mp2p_icp_hip::check(mh_place_describe(d.handle(), &p, desc.data(), MH_MEM_HOST), "mh_place_describe");
    return desc2array(desc, p); },
        py::arg("layer"), py::arg("n_rings") = 20, py::arg("n_sectors") = 64, py::arg("min_range") = 1.0f, py::arg("max_range") = 80.0f,
        py::arg("z_min") = -3.0f, py::arg("z_max") = 27.0f);
  // the key-frame decision on its own (host logic only: testable without a device; the driver holds one)
  py::class_<mola_hip::KeyFrameStore>(m, "KeyFrameStore")
      .def(py::init<bool>(), py::arg("measure_from_last_kf_only") = false)
      .def("decide", [](mola_hip::KeyFrameStore& s, bool first_scan, bool icp_good, std::vector<double> pose, double min_translation,
                        double min_rotation_deg, bool add_non_keyframes_too) {
        if (pose.size() != 12) throw std::runtime_error("need 12 values");
        CPose3D P; std::copy(pose.begin(), pose.end(), P.T);
        const auto v = s.decide(first_scan, icp_good, P, min_translation, min_rotation_deg, add_non_keyframes_too);
        return py::make_tuple(v.stored, v.keyframe); },
           py::arg("first_scan"), py::arg("icp_good"), py::arg("pose"), py::arg("min_translation"), py::arg("min_rotation_deg"),
           py::arg("add_non_keyframes_too") = false)
      .def("reset", [](mola_hip::KeyFrameStore& s) { s.reset(); });
  // ---- stand-alone odometry driver
  using mola_hip::LidarOdometry;
  auto rec2dict = [](const LidarOdometry::ScanRecord& r) {
    py::dict d;
    d["timestamp"] = r.timestamp; d["dropped"] = r.dropped; d["first_scan"] = r.first_scan; d["icp_run"] = r.icp_run;
    d["icp_good"] = r.icp_good; d["had_motion_model"] = r.had_motion_model; d["map_updated"] = r.map_updated;
    d["restarted"] = r.restarted;
    d["pose"] = std::vector<double>(r.pose.T, r.pose.T + 12);
    d["init_guess"] = std::vector<double>(r.init_guess.T, r.init_guess.T + 12);
    d["goodness"] = r.goodness; d["sigma"] = r.sigma; d["estimated_sensor_max_range"] = r.estimated_sensor_max_range;
    d["instantaneous_sensor_max_range"] = r.instantaneous_sensor_max_range;
    d["icp_iterations"] = r.icp_iterations; d["twist_corrections"] = r.twist_corrections; d["align_calls"] = r.align_calls;
    d["termination"] = r.termination; d["n_raw"] = r.n_raw; d["n_for_map"] = r.n_for_map; d["n_for_icp"] = r.n_for_icp;
    d["n_map_points"] = r.n_map_points; d["n_map_voxels"] = r.n_map_voxels;
    d["twist"] = std::vector<double>{r.twist.vx, r.twist.vy, r.twist.vz, r.twist.wx, r.twist.wy, r.twist.wz};
    d["decim_map_resolution"] = r.decim_map_resolution; d["decim_icp_resolution"] = r.decim_icp_resolution;
    d["map_voxel_size"] = r.map_voxel_size;
    d["layer_sizes"] = r.layer_sizes;
    d["waiting"] = r.waiting; d["ignored"] = r.ignored; d["n_sensors"] = r.n_sensors; d["sensor_labels"] = r.sensor_labels;
    d["relocalization_tried"] = r.relocalization_tried; d["relocalized"] = r.relocalized; d["reloc_candidates"] = r.reloc_candidates;
    d["reloc_best_n_paired"] = r.reloc_best_n_paired; d["reloc_best_quality"] = r.reloc_best_quality; d["reloc_ranks"] = r.reloc_ranks;
    d["simplemap_keyframe"] = r.simplemap_keyframe; d["simplemap_frame"] = r.simplemap_frame;
    d["place_tried"] = r.place_tried; d["place_frames"] = r.place_frames; d["place_shifts"] = r.place_shifts; d["place_dists"] = r.place_dists;
    d["loop_tried"] = r.loop_tried; d["loop_closed"] = r.loop_closed;
    py::list loop_pairs;
    for (const auto& p : r.loop_pairs) loop_pairs.append(py::make_tuple(p.i, p.j, p.quality, p.accepted));
    d["loop_pairs"] = loop_pairs;
    d["loop_correction_trans"] = r.loop_correction_trans; d["loop_correction_rot"] = r.loop_correction_rot;
    d["loop_rebuilt_frames"] = r.loop_rebuilt_frames;
    d["lost"] = r.lost; d["recovery_attempt"] = r.recovery_attempt; d["recovery_succeeded"] = r.recovery_succeeded; d["bad_streak"] = r.bad_streak;
    d["recovery_gave_up"] = r.recovery_gave_up;
    d["map_cleaned"] = r.map_cleaned;
    d["gyro_deskew"] = r.gyro_deskew; d["gyro_segments"] = r.gyro_segments;
    return d;
  };
  auto lost2dict = [](const mola_hip::LostRecoveryOptions& o) {
    py::dict d;
    d["enabled"] = o.enabled; d["bad_scans_to_lost"] = o.bad_scans_to_lost; d["method"] = o.method; d["near_sigma_xy"] = o.near_sigma_xy;
    d["near_sigma_yaw_deg"] = o.near_sigma_yaw_deg; d["retry_every_n_scans"] = o.retry_every_n_scans; d["max_attempts"] = o.max_attempts;
    return d;
  };
  // the online_map_cleaning: block (mola_lidar_odometry_hip/LiveMapCleaning.h) as a dict
  auto live2dict = [](const mola_hip::OnlineMapCleaningOptions& o) {
    py::dict d;
    d["enabled"] = o.enabled;
    d["n_rings"] = o.n_rings; d["n_sectors"] = o.n_sectors; d["el_min_deg"] = o.el_min_deg; d["el_max_deg"] = o.el_max_deg;
    d["min_range"] = o.min_range; d["max_range"] = o.max_range; d["rel_margin"] = o.rel_margin;
    d["origin_x"] = o.origin[0]; d["origin_y"] = o.origin[1]; d["origin_z"] = o.origin[2];
    d["win_rings"] = o.win_rings; d["win_sectors"] = o.win_sectors; d["max_view_distance"] = o.max_view_distance;
    d["max_views"] = o.max_views; d["min_through_votes"] = o.min_through_votes; d["agree_weight"] = o.agree_weight;
    d["every_n_updates"] = o.every_n_updates; d["view_layer"] = o.view_layer; d["target_maps"] = o.target_maps;
    const mh_clean_params p = o.deviceParams();  // what the device is given: the floats of mh_clean_params
    d["device_params"] = py::make_tuple(p.n_rings, p.n_sectors, p.el_min, p.el_max, p.min_range, p.max_range, p.rel_margin,
                                        py::make_tuple(p.origin[0], p.origin[1], p.origin[2]), p.win_rings, p.win_sectors);
    return d;
  };
  // `options`: a pipeline Config, the YAML text of one, or None (the defaults)
  auto live_opts = [](const py::object& options) {
    using mola_hip::OnlineMapCleaningOptions;
    if (options.is_none()) return OnlineMapCleaningOptions::FromConfig(Config::FromYamlText(""));
    if (py::isinstance<py::str>(options)) return OnlineMapCleaningOptions::FromConfig(Config::FromYamlText(options.cast<std::string>()));
    return OnlineMapCleaningOptions::FromConfig(options.cast<const Config&>());
  };
  // the gyro_deskew: block (mola_lidar_odometry_hip/GyroDeskew.h) as a dict; `options` as above
  auto gyro_opts = [](const py::object& options) {
    using mola_hip::GyroDeskewOptions;
    if (options.is_none()) return GyroDeskewOptions::FromConfig(Config::FromYamlText(""));
    if (py::isinstance<py::str>(options)) return GyroDeskewOptions::FromConfig(Config::FromYamlText(options.cast<std::string>()));
    return GyroDeskewOptions::FromConfig(options.cast<const Config&>());
  };
  auto gyro2dict = [](const mola_hip::GyroDeskewOptions& o) {
    py::dict d;
    d["enabled"] = o.enabled; d["window"] = std::vector<double>(o.window, o.window + 2); d["segments"] = o.segments; d["max_gap"] = o.max_gap;
    d["time_zero_offset"] = o.time_zero_offset; d["gyro_bias"] = std::vector<double>(o.gyro_bias, o.gyro_bias + 3);
    d["sensor_rotation"] = std::vector<double>(o.sensor_rotation, o.sensor_rotation + 9); d["buffer_seconds"] = o.buffer_seconds;
    return d;
  };
  m.def("gyro_deskew_options", [gyro2dict, gyro_opts](const py::object& options) { return gyro2dict(gyro_opts(options)); }, py::arg("options") = py::none());
  // the host rule on its own: samples (t [n], w [n, 3]) pushed into a GyroBuffer of the options' length in order, then
  // build_motion_table -> None (no coverage) or dict(knots [K], R [K, 3, 3], w [K, 3], v [3]); "dropped" / "kept" ride along
  m.def("gyro_motion_table", [gyro_opts](py::array_t<double, py::array::c_style | py::array::forcecast> t,
                                         py::array_t<double, py::array::c_style | py::array::forcecast> w, double timestamp, const py::object& options,
                                         std::vector<double> v) -> py::object {
    if (t.ndim() != 1 || w.ndim() != 2 || w.shape(1) != 3 || w.shape(0) != t.shape(0)) throw std::runtime_error("gyro_motion_table: t must be [n] and w [n, 3]");
    if (v.size() != 3) throw std::runtime_error("gyro_motion_table: v has 3 values");
    const mola_hip::GyroDeskewOptions o = gyro_opts(options);
    mola_hip::GyroBuffer buf(o.buffer_seconds);
    for (py::ssize_t k = 0; k < t.shape(0); k++) buf.push(t.data()[k], w.data() + 3 * k);
    const auto tab = mola_hip::build_motion_table(buf, timestamp, o, v.data());
    py::dict d;
    d["dropped"] = buf.dropped(); d["kept"] = buf.size();
    if (!tab) { d["table"] = py::none(); return d; }
    const py::ssize_t K = (py::ssize_t)tab->segments.size();
    py::array_t<double> knots(K), R({K, (py::ssize_t)3, (py::ssize_t)3}), ws({K, (py::ssize_t)3});
    for (py::ssize_t s = 0; s < K; s++) {
      knots.mutable_data()[s] = tab->segments[(size_t)s].knot;
      std::copy(tab->segments[(size_t)s].R, tab->segments[(size_t)s].R + 9, R.mutable_data() + 9 * s);
      std::copy(tab->segments[(size_t)s].w, tab->segments[(size_t)s].w + 3, ws.mutable_data() + 3 * s);
    }
    py::dict tb;
    tb["knots"] = knots; tb["R"] = R; tb["w"] = ws; tb["v"] = std::vector<double>(tab->v, tab->v + 3);
    d["table"] = tb;
    return d; }, py::arg("t"), py::arg("w"), py::arg("timestamp"), py::arg("options") = py::none(), py::arg("v") = std::vector<double>{0, 0, 0});
  // the command line's --gyro-file text -> (t [n], w [n, 3])
  m.def("parse_gyro_text", [](const std::string& text) {
    const auto g = mola_hip::parse_gyro_text(text);
    py::array_t<double> t((py::ssize_t)g.size()), w({(py::ssize_t)g.size(), (py::ssize_t)3});
    for (size_t k = 0; k < g.size(); k++) { t.mutable_data()[k] = g[k].t; std::copy(g[k].w, g[k].w + 3, w.mutable_data() + 3 * k); }
    return py::make_tuple(t, w); }, py::arg("text"));
  m.def("online_map_cleaning_options", [live2dict, live_opts](const py::object& options) { return live2dict(live_opts(options)); },
        py::arg("options") = py::none());
  // the ring rule on its own (host logic only; the driver's LiveMapCleaner holds one): poses [K, 12] of K local map updates in a
  // row -> per update (slot, due, neighbour slots)
  m.def("live_ring_fold", [live_opts](py::array_t<double, py::array::c_style | py::array::forcecast> poses, const py::object& options) {
    if (poses.ndim() != 2 || poses.shape(1) != 12) throw std::runtime_error("live_ring_fold: poses must be [K, 12]");
    const mola_hip::OnlineMapCleaningOptions o = live_opts(options);
    mola_hip::LiveRing ring(o.max_views, o.every_n_updates);
    py::list out;
    for (py::ssize_t k = 0; k < poses.shape(0); k++) {
      const double* P = poses.data() + 12 * k;
      const mola_hip::LiveRing::Step st = ring.put(P);
      out.append(py::make_tuple(st.slot, st.due, st.due ? ring.neighbours(P, o.max_view_distance) : std::vector<uint32_t>()));
    }
    return out; }, py::arg("poses"), py::arg("options") = py::none());
  // the lost_recovery: block of a pipeline Config as a dict (an absent block: the defaults)
  m.def("lost_recovery_options", [lost2dict](const Config& c) { return lost2dict(mola_hip::LostRecoveryOptions::FromConfig(c)); });
  // the state machine of lost_recovery: on its own (host logic only; the driver holds one).  scan(icp_good, outcome, caller_request, near_fits):
  // one scan that reaches registration, in the driver's order -- the caller may have placed a request before it (caller_request); a
  // pending request is served with `outcome` (a failed caller's request stays pending); the gate sees icp_good (None: the alignment
  // did not run, or the scan restarted the map); the driver's own request is placed when due (near_fits: a `near`
  // attempt's grid stays within max_candidates; false: skipped) -> the record fields, and what was placed.
  struct LostRecoveryHook {
    mola_hip::LostRecovery m;
    bool pending = false;
  };
  py::class_<LostRecoveryHook>(m, "LostRecovery")
      .def(py::init([](const Config& c) { return LostRecoveryHook{mola_hip::LostRecovery(mola_hip::LostRecoveryOptions::FromConfig(c)), false}; }))
      .def("scan", [](LostRecoveryHook& h, std::optional<bool> icp_good, bool outcome, bool caller_request, bool near_fits) {
        mola_hip::LostRecovery::Fields f;
        if (caller_request) {
          h.pending = true;
          h.m.callerRequested();
        }
        f.lost = h.m.lost();
        f.bad_streak = h.m.badStreak();
        if (h.pending) {
          const bool clear = h.m.served(outcome, f);
          if (outcome || clear) h.pending = false;
        }
        if (icp_good) h.m.gate(*icp_good, f);
        const uint32_t kind = h.m.due(h.pending, near_fits);
        if (kind) {
          h.pending = true;
          h.m.placed(kind);
        }
        py::dict d;
        d["lost"] = f.lost; d["recovery_attempt"] = f.recovery_attempt; d["recovery_succeeded"] = f.recovery_succeeded; d["bad_streak"] = f.bad_streak;
        d["recovery_gave_up"] = h.m.gaveUp(); d["placed"] = kind; d["pending"] = h.pending;
        return d; }, py::arg("icp_good"), py::arg("outcome") = false, py::arg("caller_request") = false, py::arg("near_fits") = true)
      .def("reset", [](LostRecoveryHook& h) { h.m.reset(); h.pending = false; })
      .def("isLost", [](const LostRecoveryHook& h) { return h.m.lost(); })
      .def("timesLost", [](const LostRecoveryHook& h) { return h.m.timesLost(); })
      .def("recoveryAttempts", [](const LostRecoveryHook& h) { return h.m.attempts(); })
      .def("timesRecovered", [](const LostRecoveryHook& h) { return h.m.timesRecovered(); })
      .def("skipped", [](const LostRecoveryHook& h) { return h.m.skipped(); })
      .def("gaveUp", [](const LostRecoveryHook& h) { return h.m.gaveUp(); });
  py::class_<LidarOdometry> lo_class(m, "LidarOdometry", py::dynamic_attr());
  lo_class
      .def(py::init([](int device, bool own_context) {
             // default: the process-wide context on device 0; device >= 0 / own_context: a context (stream + scratch) of
             // its own on that device -- one per GPU rank, and required when several drivers run in threads of one process
             if (device < 0 && !own_context) return std::make_unique<LidarOdometry>();
             return std::make_unique<LidarOdometry>(std::make_shared<DeviceContext>(device < 0 ? 0 : device)); }),
           py::arg("device") = -1, py::arg("own_context") = false)
      .def("initialize", &LidarOdometry::initialize)
      .def("reset", &LidarOdometry::reset)
      .def("onLidar", [rec2dict](LidarOdometry& lo, double stamp, py::array_t<float, py::array::c_style | py::array::forcecast> xyz,
                                 std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                                 std::array<int, 3> xyz_fields, int t_field, int i_field) {
        // [n,3] points or [n,k] float32 records (a KITTI .bin is [n,4]; a PointCloud2 payload of float fields likewise):
        // the rows go to the device as they are and are split into channels there.  xyz_fields / t_field / i_field = column
        // indices of the coordinates / of a per-point time stamp (-1: none, or the separate array `t`) / of the intensity
        // (-1: none; read only by a pipeline with intensity filters, setIntensityInput)
        if (xyz.ndim() != 2 || xyz.shape(1) < 3) throw std::runtime_error("xyz must be [n,3] (or [n,k>=3] records)");
        const size_t n = (size_t)xyz.shape(0), k = (size_t)xyz.shape(1);
        for (int f : xyz_fields)
          if (f < 0 || (size_t)f >= k) throw std::runtime_error("xyz_fields out of range");
        if (t_field >= (int)k) throw std::runtime_error("t_field out of range");
        if (i_field >= (int)k) throw std::runtime_error("i_field out of range");
        const float* tp = nullptr;
        if (t) {
          if ((size_t)t->size() != n) throw std::runtime_error("t must have n entries");
          tp = t->data();
        }
        {
          py::gil_scoped_release nogil;  // the numpy buffers are only read through their pointers: other drivers' threads may run
          (void)lo.onLidarInterleaved(stamp, xyz.data(), n, k * sizeof(float), 4u * (size_t)xyz_fields[0],
                                       4u * (size_t)xyz_fields[1], 4u * (size_t)xyz_fields[2],
                                       t_field >= 0 ? 4ll * t_field : -1ll, tp, i_field >= 0 ? 4ll * i_field : -1ll);
        }
        return rec2dict(lo.records().back()); },  // (records(): the map counters of this record, read back now)
           py::arg("timestamp"), py::arg("xyz"), py::arg("t") = std::nullopt,
           py::arg("xyz_fields") = std::array<int, 3>{0, 1, 2}, py::arg("t_field") = -1, py::arg("i_field") = -1)
      .def("onLidarFrom", [rec2dict](LidarOdometry& lo, const std::string& label, double stamp,
                                     py::array_t<float, py::array::c_style | py::array::forcecast> xyz,
                                     std::optional<py::array_t<float, py::array::c_style | py::array::forcecast>> t,
                                     std::array<int, 3> xyz_fields, int t_field, int i_field, std::optional<std::vector<double>> sensor_pose) {
        // one observation of a labelled sensor of a rig, points in the SENSOR frame (arguments as onLidar's); sensor_pose: 12
        // values, row-major 3x4, the sensor on the vehicle (default: identity)
        if (xyz.ndim() != 2 || xyz.shape(1) < 3) throw std::runtime_error("xyz must be [n,3] (or [n,k>=3] records)");
        const size_t n = (size_t)xyz.shape(0), k = (size_t)xyz.shape(1);
        for (int f : xyz_fields)
          if (f < 0 || (size_t)f >= k) throw std::runtime_error("xyz_fields out of range");
        if (t_field >= (int)k) throw std::runtime_error("t_field out of range");
        if (i_field >= (int)k) throw std::runtime_error("i_field out of range");
        if (sensor_pose && sensor_pose->size() != 12) throw std::runtime_error("sensor_pose must hold 12 values (row-major 3x4)");
        const float* tp = nullptr;
        if (t) {
          if ((size_t)t->size() != n) throw std::runtime_error("t must have n entries");
          tp = t->data();
        }
        {
          py::gil_scoped_release nogil;
          (void)lo.onLidarFrom(label, sensor_pose ? sensor_pose->data() : nullptr, stamp, xyz.data(), n, k * sizeof(float),
                               4u * (size_t)xyz_fields[0], 4u * (size_t)xyz_fields[1], 4u * (size_t)xyz_fields[2],
                               t_field >= 0 ? 4ll * t_field : -1ll, tp, i_field >= 0 ? 4ll * i_field : -1ll);
        }
        return rec2dict(lo.records().back()); },
           py::arg("label"), py::arg("timestamp"), py::arg("xyz"), py::arg("t") = std::nullopt,
           py::arg("xyz_fields") = std::array<int, 3>{0, 1, 2}, py::arg("t_field") = -1, py::arg("i_field") = -1,
           py::arg("sensor_pose") = std::nullopt)
      .def("onDepthImage", [rec2dict](LidarOdometry& lo, double stamp, py::array range, double fx, double fy, double cx, double cy,
                                      double range_units, bool range_is_depth, std::optional<std::vector<double>> sensor_pose) {
        // [rows, cols] uint16 range image, 0 = no return; read through its pointer: a C-contiguous uint16 array only (anything
        // else is rejected instead of converted).  sensor_pose: 12 values, row-major 3x4 (default: identity)
        if (!py::dtype::of<uint16_t>().is(range.dtype()) || !(range.flags() & py::array::c_style) || range.ndim() != 2)
          throw std::runtime_error("range must be a C-contiguous [rows, cols] uint16 array");
        if (sensor_pose && sensor_pose->size() != 12) throw std::runtime_error("sensor_pose must hold 12 values (row-major 3x4)");
        mh_range_image_params cam;
        memset(&cam, 0, sizeof(cam));
        cam.rows = (uint32_t)range.shape(0);
        cam.cols = (uint32_t)range.shape(1);
        cam.fx = (float)fx; cam.fy = (float)fy; cam.cx = (float)cx; cam.cy = (float)cy;
        cam.range_units = (float)range_units;
        cam.range_is_depth = range_is_depth ? 1u : 0u;
        for (int i = 0; i < 12; i++) cam.sensor_pose[i] = sensor_pose ? (*sensor_pose)[i] : (i % 5 == 0 ? 1.0 : 0.0);
        {
          py::gil_scoped_release nogil;
          (void)lo.onDepthImage(stamp, static_cast<const uint16_t*>(range.data()), cam);
        }
        return rec2dict(lo.records().back()); },
           py::arg("timestamp"), py::arg("range"), py::arg("fx"), py::arg("fy"), py::arg("cx"), py::arg("cy"),
           py::arg("range_units") = 0.001, py::arg("range_is_depth") = true, py::arg("sensor_pose") = std::nullopt)
      .def("localMapClasses", &LidarOdometry::localMapClasses)
      .def("saveLocalMaps", &LidarOdometry::saveLocalMaps, py::call_guard<py::gil_scoped_release>())
      .def("keyFrames", [kfset2dict](const LidarOdometry& lo) { return kfset2dict(lo.keyFrames()); })
      .def("saveKeyFrames", &LidarOdometry::saveKeyFrames, py::call_guard<py::gil_scoped_release>())
      .def("simplemapOptions", [](const LidarOdometry& lo) {
        const auto& o = lo.params().simplemap;
        py::dict d;
        d["generate"] = o.generate; d["min_translation_between_keyframes"] = o.min_translation_between_keyframes;
        d["min_rotation_between_keyframes"] = o.min_rotation_between_keyframes; d["measure_from_last_kf_only"] = o.measure_from_last_kf_only;
        d["add_non_keyframes_too"] = o.add_non_keyframes_too; d["generate_lazy_load_scan_files"] = o.generate_lazy_load_scan_files;
        d["save_gnss_max_age"] = o.save_gnss_max_age; d["save_final_map_to_file"] = o.save_final_map_to_file;
        d["load_existing_simple_map"] = o.load_existing_simple_map;
        return d; })
      // mean: 12 values, row-major [R|t]; cov: 36 values, row-major 6x6 in (x, y, z, yaw, pitch, roll)
      .def("relocalizeNearPose", [](LidarOdometry& lo, std::vector<double> mean, std::vector<double> cov) {
        if (mean.size() != 12 || cov.size() != 36) throw std::runtime_error("need 12 pose values and 36 covariance values");
        CPose3D P; std::copy(mean.begin(), mean.end(), P.T);
        lo.relocalizeNearPose(P, cov.data()); })
      .def("relocalizeInKeyFrames", &LidarOdometry::relocalizeInKeyFrames)
      .def("relocalizationPending", &LidarOdometry::relocalizationPending)
      .def("lostRecoveryOptions", [lost2dict](const LidarOdometry& lo) { return lost2dict(lo.lostRecoveryOptions()); })
      .def("onlineMapCleaningOptions", [live2dict](const LidarOdometry& lo) { return live2dict(lo.onlineMapCleaningOptions()); })
      .def("mapPointsErased", &LidarOdometry::mapPointsErased)
      .def("onGyro", [](LidarOdometry& lo, double t, std::vector<double> w) {
        if (w.size() != 3) throw std::runtime_error("onGyro: w has 3 values");
        lo.onGyro(t, w.data()); })
      .def("gyroDeskewOptions", [gyro2dict](const LidarOdometry& lo) { return gyro2dict(lo.gyroDeskewOptions()); })
      .def("scansGyroDeskewed", &LidarOdometry::scansGyroDeskewed)
      .def("gyroSamplesDropped", &LidarOdometry::gyroSamplesDropped)
      .def("isLost", &LidarOdometry::isLost)
      .def("timesLost", &LidarOdometry::timesLost)
      .def("recoveryAttempts", &LidarOdometry::recoveryAttempts)
      .def("timesRecovered", &LidarOdometry::timesRecovered)
      .def("recoveryGaveUp", &LidarOdometry::recoveryGaveUp)
      .def("lastRecoveryError", [](const LidarOdometry& lo) { return lo.lastRecoveryError(); })
      .def("initialLocalization", [](const LidarOdometry& lo) {
        const auto& il = lo.initialLocalization();
        py::dict d;
        d["enabled"] = il.enabled; d["method"] = il.method; d["relocalize"] = il.relocalize;
        d["fixed_initial_pose"] = std::vector<double>{il.fixed_initial_pose.x, il.fixed_initial_pose.y, il.fixed_initial_pose.z,
                                                      il.fixed_initial_pose.yaw, il.fixed_initial_pose.pitch, il.fixed_initial_pose.roll};
        d["relocalize_sigmas"] = std::vector<double>(il.relocalize_sigmas, il.relocalize_sigmas + 3);
        return d; })
      .def("relocalizationOptions", [](const LidarOdometry& lo) {
        const auto& r = lo.relocalizationOptions();
        py::dict d;
        d["score_threshold"] = r.score_threshold; d["step_xy"] = r.step_xy; d["step_yaw_deg"] = r.step_yaw_deg; d["sigmas"] = r.sigmas;
        d["refine_top_k"] = r.refine_top_k; d["max_candidates"] = r.max_candidates;
        d["place_rings"] = r.place_rings; d["place_sectors"] = r.place_sectors; d["place_min_range"] = r.place_min_range;
        d["place_max_range"] = r.place_max_range; d["place_z_min"] = r.place_z_min; d["place_z_max"] = r.place_z_max;
        d["place_top_k"] = r.place_top_k; d["place_sigma_xy"] = r.place_sigma_xy; d["place_sigma_yaw_deg"] = r.place_sigma_yaw_deg;
        return d; })
      .def("loadExistingLocalMap", [](const LidarOdometry& lo) { return lo.params().load_existing_local_map; })
      .def("setIntensityInput", &LidarOdometry::setIntensityInput)
      .def("setAlignBatcher", &LidarOdometry::setAlignBatcher)
      .def("prefetch", [](py::object self, py::array xyz_any, std::optional<py::array> t_any,
                          std::array<int, 3> xyz_fields, int t_field, int i_field) {
        // announce the NEXT scan (same arguments as the onLidar call that will follow): upload + first filter pass run
        // on a second stream while the current scan is registered.  The worker thread reads the caller's buffers, so
        // no hidden temporary may stand in for them: float32, C-contiguous arrays only (anything else is rejected
        // instead of converted), kept alive on the object -- the announced scan AND the one whose worker may still be
        // running (it is joined by the onLidar call that picks it up, which comes before the next prefetch but one).
        auto strict = [](const py::array& a, const char* what) {
          if (!py::dtype::of<float>().is(a.dtype()) || !(a.flags() & py::array::c_style))
            throw std::runtime_error(std::string(what) + " must be a C-contiguous float32 array (prefetch reads it from a worker thread)");
        };
        strict(xyz_any, "xyz");
        if (t_any) strict(*t_any, "t");
        auto xyz = py::array_t<float, py::array::c_style>::ensure(xyz_any);
        std::optional<py::array_t<float, py::array::c_style>> t;
        if (t_any) t = py::array_t<float, py::array::c_style>::ensure(*t_any);
        if (!xyz || (t_any && !*t)) throw std::runtime_error("prefetch: unusable array");
        if (xyz.data() != xyz_any.data() || (t && t->data() != t_any->data())) throw std::runtime_error("prefetch: array was copied");
        LidarOdometry& lo = self.cast<LidarOdometry&>();
        if (xyz.ndim() != 2 || xyz.shape(1) < 3) throw std::runtime_error("xyz must be [n,3] (or [n,k>=3] records)");
        const size_t n = (size_t)xyz.shape(0), k = (size_t)xyz.shape(1);
        for (int f : xyz_fields)
          if (f < 0 || (size_t)f >= k) throw std::runtime_error("xyz_fields out of range");
        if (t_field >= (int)k) throw std::runtime_error("t_field out of range");
        if (i_field >= (int)k) throw std::runtime_error("i_field out of range");
        const float* tp = nullptr;
        if (t) {
          if ((size_t)t->size() != n) throw std::runtime_error("t must have n entries");
          tp = t->data();
        }
        lo.prefetchInterleaved(xyz.data(), n, k * sizeof(float), 4u * (size_t)xyz_fields[0], 4u * (size_t)xyz_fields[1],
                               4u * (size_t)xyz_fields[2], t_field >= 0 ? 4ll * t_field : -1ll, tp, i_field >= 0 ? 4ll * i_field : -1ll);
        if (py::hasattr(self, "_prefetch_keepalive")) self.attr("_prefetch_inflight") = self.attr("_prefetch_keepalive");
        self.attr("_prefetch_keepalive") = py::make_tuple(xyz, t ? py::object(*t) : py::none()); },
           py::arg("xyz"), py::arg("t") = std::nullopt, py::arg("xyz_fields") = std::array<int, 3>{0, 1, 2},
           py::arg("t_field") = -1, py::arg("i_field") = -1)
      .def("records", [rec2dict](const LidarOdometry& lo) { py::list l; for (auto& r : lo.records()) l.append(rec2dict(r)); return l; })
      .def("trajectory", [](const LidarOdometry& lo) {
        py::list l;
        for (auto& [t, p] : lo.estimatedTrajectory()) l.append(py::make_tuple(t, std::vector<double>(p.T, p.T + 12)));
        return l; })
      .def("saveTrajectoryTUM", &LidarOdometry::saveTrajectoryTUM)
      .def("correctedTrajectory", [](const LidarOdometry& lo) {
        py::list l;
        for (auto& [t, p] : lo.correctedTrajectory()) l.append(py::make_tuple(t, std::vector<double>(p.T, p.T + 12)));
        return l; })
      .def("saveCorrectedTrajectoryTUM", &LidarOdometry::saveCorrectedTrajectoryTUM)
      .def("rawKeyFrames", [kfset2dict](const LidarOdometry& lo) { return kfset2dict(lo.rawKeyFrames()); })
      .def("loopCloser", [](const LidarOdometry& lo) { return std::const_pointer_cast<mola_hip::OnlineLoopCloser>(lo.loopCloser()); },
           py::keep_alive<0, 1>())  // (the closer reads the layers of the driver's key-frame store)
      .def("dynamicVariables", &LidarOdometry::dynamicVariables)
      .def("describePipeline", &LidarOdometry::describePipeline)
      .def("profile", [](const LidarOdometry& lo) { return lo.profile(); })
      .def("localMapSize", [](const LidarOdometry& lo) { return lo.localMap() ? lo.localMap()->size() : 0; })
      .def("localMapSizes", &LidarOdometry::localMapSizes)
      // debug accessors (they synchronise and copy: tests only)
      .def("localMapStats", [](const LidarOdometry& lo) {
        py::dict d;
        for (const auto& [name, s] : lo.localMapStats()) d[py::str(name)] = py::make_tuple(s.n_points, s.n_voxels, s.voxel_size);
        return d; })
      .def("downloadLayer", [](const LidarOdometry& lo, const std::string& name) {
        const LidarOdometry::LayerDump l = lo.downloadLayer(name);
        const py::ssize_t n = (py::ssize_t)l.x.size();
        py::array_t<float> xyz({n, (py::ssize_t)3});
        auto w = xyz.mutable_unchecked<2>();
        for (py::ssize_t i = 0; i < n; i++) { w(i, 0) = l.x[i]; w(i, 1) = l.y[i]; w(i, 2) = l.z[i]; }
        py::dict d;
        d["xyz"] = xyz;
        d["t"] = py::array_t<float>(n, l.t.data());
        d["src_idx"] = py::array_t<uint32_t>(n, l.src_idx.data());
        d["intensity"] = l.intensity.empty() ? py::object(py::none()) : py::object(py::array_t<float>(n, l.intensity.data()));
        d["alive"] = l.alive;
        return d; })
      .def("downloadMap", [](const LidarOdometry& lo, const std::string& name) {
        const LidarOdometry::MapDump m = lo.downloadMap(name);
        const py::ssize_t n = (py::ssize_t)m.x.size(), v = (py::ssize_t)m.vox_count.size();
        py::array_t<float> xyz({n, (py::ssize_t)3});
        auto w = xyz.mutable_unchecked<2>();
        for (py::ssize_t i = 0; i < n; i++) { w(i, 0) = m.x[i]; w(i, 1) = m.y[i]; w(i, 2) = m.z[i]; }
        py::array_t<int32_t> keys({v, (py::ssize_t)3});
        if (v) std::copy(m.vox_keys.begin(), m.vox_keys.end(), keys.mutable_data());
        py::dict d;
        d["xyz"] = xyz;
        d["src_idx"] = py::array_t<uint32_t>(n, m.src_idx.data());
        d["vox_keys"] = keys;
        d["vox_first"] = py::array_t<uint32_t>(v, m.vox_first.data());
        d["vox_count"] = py::array_t<uint32_t>(v, m.vox_count.data());
        return d; });
  lo_class.def("downloadVoxelMap", [](const LidarOdometry& lo, const std::string& name) {
    const LidarOdometry::VoxelMapDump v = lo.downloadVoxelMap(name);
    const py::ssize_t n = (py::ssize_t)v.logodds.size();
    py::array_t<int32_t> keys({n, (py::ssize_t)3});
    if (n) std::copy(v.keys.begin(), v.keys.end(), keys.mutable_data());
    py::dict d;
    d["keys"] = keys;
    d["logodds"] = py::array_t<int32_t>(n, v.logodds.data());
    d["search_voxel_size"] = v.search_voxel_size;
    return d; });
  // the grouping rule of a rig on its own (host logic only: testable without a device; the driver holds one)
  py::class_<mola_hip::SensorSync>(m, "SensorSync")
      .def(py::init<uint32_t, double>(), py::arg("lidar_count") = 1, py::arg("max_time_offset") = 25e-3)
      .def("push", [](mola_hip::SensorSync& s, const std::string& label, double stamp) -> py::object {
        const auto g = s.push(label, stamp);
        if (!g) return py::none();
        return py::make_tuple(g->labels, g->dts, g->discarded); })
      .def("waiting", &mola_hip::SensorSync::waiting)
      .def("clear", &mola_hip::SensorSync::clear);
  py::class_<AlignBatcher, std::shared_ptr<AlignBatcher>>(m, "AlignBatcher")
      .def(py::init<size_t>(), py::arg("participants"))
      .def("leave", [](AlignBatcher& b) { b.leave(); }, py::call_guard<py::gil_scoped_release>())
      .def("batches", &AlignBatcher::batches)
      .def("jobs", &AlignBatcher::jobs);
  // ---- the local-map file on host arrays (molahip_host/local_map_file.h): a map is a dict with the keys name, class_name,
  // params (voxel_size, max_points_per_voxel, index_mode, min_distance_between_points, ndt_max_eigen_ratio, ndt_min_points,
  // far_voxel_metric), remove_voxels_farther_than, n_offered, xyz [n, 3] float32, src_idx [n] uint32
  m.def("write_local_map_file", [](const std::string& path, const std::vector<py::dict>& maps) {
    std::vector<molahip_host::LocalMapRecord> recs;
    for (const py::dict& d : maps) {
      molahip_host::LocalMapRecord r;
      r.name = d["name"].cast<std::string>();
      r.class_name = d["class_name"].cast<std::string>();
      const py::dict p = d["params"].cast<py::dict>();
      r.params.voxel_size = p["voxel_size"].cast<float>();
      r.params.max_points_per_voxel = p["max_points_per_voxel"].cast<uint32_t>();
      r.params.index_mode = p["index_mode"].cast<uint32_t>();
      r.params.min_distance_between_points = p["min_distance_between_points"].cast<float>();
      r.params.ndt_max_eigen_ratio = p["ndt_max_eigen_ratio"].cast<float>();
      r.params.ndt_min_points = p["ndt_min_points"].cast<uint32_t>();
      r.params.far_voxel_metric = p["far_voxel_metric"].cast<uint32_t>();
      r.remove_voxels_farther_than = d["remove_voxels_farther_than"].cast<float>();
      r.n_offered = d["n_offered"].cast<uint64_t>();
      auto xyz = d["xyz"].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
      auto src = d["src_idx"].cast<py::array_t<uint32_t, py::array::c_style | py::array::forcecast>>();
      if (xyz.ndim() != 2 || xyz.shape(1) != 3 || src.ndim() != 1 || src.shape(0) != xyz.shape(0))
        throw std::runtime_error("xyz must be [n, 3] and src_idx [n]");
      const py::ssize_t n = xyz.shape(0);
      auto a = xyz.unchecked<2>();
      r.x.resize(n); r.y.resize(n); r.z.resize(n);
      for (py::ssize_t i = 0; i < n; i++) { r.x[i] = a(i, 0); r.y[i] = a(i, 1); r.z[i] = a(i, 2); }
      r.src_idx.assign(src.data(), src.data() + n);
      recs.push_back(std::move(r));
    }
    molahip_host::write_local_map_file(path, recs); });
  m.def("read_local_map_file", [](const std::string& path) {
    py::list out;
    for (const auto& r : molahip_host::read_local_map_file(path)) {
      py::dict d, p;
      d["name"] = r.name; d["class_name"] = r.class_name;
      p["voxel_size"] = r.params.voxel_size; p["max_points_per_voxel"] = r.params.max_points_per_voxel; p["index_mode"] = r.params.index_mode;
      p["min_distance_between_points"] = r.params.min_distance_between_points; p["ndt_max_eigen_ratio"] = r.params.ndt_max_eigen_ratio;
      p["ndt_min_points"] = r.params.ndt_min_points; p["far_voxel_metric"] = r.params.far_voxel_metric;
      d["params"] = p;
      d["remove_voxels_farther_than"] = r.remove_voxels_farther_than; d["n_offered"] = r.n_offered;
      const py::ssize_t n = (py::ssize_t)r.x.size();
      py::array_t<float> xyz({n, (py::ssize_t)3});
      auto w = xyz.mutable_unchecked<2>();
      for (py::ssize_t i = 0; i < n; i++) { w(i, 0) = r.x[i]; w(i, 1) = r.y[i]; w(i, 2) = r.z[i]; }
      d["xyz"] = xyz;
      d["src_idx"] = py::array_t<uint32_t>(n, r.src_idx.data());
      out.append(d);
    }
    return out; });
  m.attr("LOCAL_MAP_FILE_VERSION") = molahip_host::kLocalMapFileVersion;
  // candidate poses of a relocalization: mean = (x, y, z, yaw, pitch, roll), cov = 36 values; returns (poses [k, 12], rows [k, 6])
  m.def("relocalization_grid", [](std::vector<double> mean, std::vector<double> cov, double step_xy, double step_yaw_rad, double sigmas,
                                  size_t max_candidates) {
    if (mean.size() != 6 || cov.size() != 36) throw std::runtime_error("need 6 pose values (x y z yaw pitch roll) and 36 covariance values");
    const TPose3D mu{mean[0], mean[1], mean[2], mean[3], mean[4], mean[5]};
    const std::vector<TPose3D> g = mola_hip::relocalization_grid(mu, cov.data(), step_xy, step_yaw_rad, sigmas, max_candidates);
    const py::ssize_t k = (py::ssize_t)g.size();
    py::array_t<double> poses({k, (py::ssize_t)12}), rows({k, (py::ssize_t)6});
    auto wp = poses.mutable_unchecked<2>();
    auto wr = rows.mutable_unchecked<2>();
    for (py::ssize_t i = 0; i < k; i++) {
      const CPose3D P(g[i]);
      for (int j = 0; j < 12; j++) wp(i, j) = P.T[j];
      const double v[6] = {g[i].x, g[i].y, g[i].z, g[i].yaw, g[i].pitch, g[i].roll};
      for (int j = 0; j < 6; j++) wr(i, j) = v[j];
    }
    return py::make_tuple(poses, rows); },
        py::arg("mean"), py::arg("cov"), py::arg("step_xy"), py::arg("step_yaw_rad"), py::arg("sigmas") = 3.0, py::arg("max_candidates") = 65536);
  // steps 2-4 of a relocalization on their own (mola_hip::score_rank_refine): candidates = TPose3D rows [k, 6]; host PointCloud
  // layers of pcLocal are uploaded to the global layer's device first (the driver's layers live there already).
  // -> {ranks, n_paired, cost (of the kept candidates), have, quality, iterations, pose [12]}
  m.def("score_rank_refine", [](ICP& icp, const Parameters& p, const metric_map_t& pcLocal, const metric_map_t& pcGlobal, const std::string& global_layer,
                                const std::string& local_layer, py::array_t<double, py::array::c_style | py::array::forcecast> candidates,
                                double score_threshold, uint32_t refine_top_k) {
    if (candidates.ndim() != 2 || candidates.shape(1) != 6) throw std::runtime_error("candidates must be [k, 6] rows of x y z yaw pitch roll");
    const auto gi = pcGlobal.layers.find(global_layer);
    auto g = gi == pcGlobal.layers.end() ? nullptr : std::dynamic_pointer_cast<HashedVoxelPointCloud>(gi->second);
    if (!g) throw std::runtime_error("score_rank_refine: no device map called '" + global_layer + "' in pcGlobal");
    metric_map_t local;
    for (const auto& [name, layer] : pcLocal.layers) {
      auto host_cloud = std::dynamic_pointer_cast<PointCloud>(layer);
      if (!host_cloud) { local.layers[name] = layer; continue; }
      auto dev = std::make_shared<DevicePointCloud>(g->context());
      dev->setPoints(host_cloud->x.data(), host_cloud->y.data(), host_cloud->z.data(), host_cloud->size());
      local.layers[name] = dev;
    }
    std::vector<TPose3D> cand((size_t)candidates.shape(0));
    auto a = candidates.unchecked<2>();
    for (size_t c = 0; c < cand.size(); c++) cand[c] = TPose3D{a(c, 0), a(c, 1), a(c, 2), a(c, 3), a(c, 4), a(c, 5)};
    mola_hip::RelocalizationRefinement r;
    {
      py::gil_scoped_release nogil;
      r = mola_hip::score_rank_refine(icp, p, local, pcGlobal, global_layer, local_layer, cand, score_threshold, refine_top_k);
    }
    std::vector<uint32_t> n_paired;
    std::vector<uint64_t> cost;
    for (const auto& s : r.scores) n_paired.push_back(s.n_paired), cost.push_back(s.cost);
    py::dict d;
    d["ranks"] = r.ranks; d["n_paired"] = n_paired; d["cost"] = cost; d["have"] = r.have; d["quality"] = r.best.quality;
    d["iterations"] = r.best.nIterations; d["pose"] = std::vector<double>(r.best.optimal_tf.mean.T, r.best.optimal_tf.mean.T + 12);
    return d; }, py::arg("icp"), py::arg("params"), py::arg("pcLocal"), py::arg("pcGlobal"), py::arg("global_layer"), py::arg("local_layer"),
        py::arg("candidates"), py::arg("score_threshold"), py::arg("refine_top_k"));
  // ---- loop closure over a key-frame set (mola_lidar_odometry_hip/LoopClosure.h)
  using mola_hip::LoopClosureOptions;
  auto opts2dict = [](const LoopClosureOptions& o) {
    py::dict d;
    d["min_travel"] = o.min_travel; d["gate_base"] = o.gate_base; d["gate_rate"] = o.gate_rate; d["max_place_dist"] = o.max_place_dist;
    d["top_k"] = o.top_k; d["min_travel_between_closures"] = o.min_travel_between_closures; d["submap_radius"] = o.submap_radius;
    d["sigma_xy"] = o.sigma_xy; d["sigma_yaw_deg"] = o.sigma_yaw_deg; d["sigma"] = o.sigma; d["min_quality"] = o.min_quality;
    d["odometry_sigma_xyz"] = o.odometry_sigma_xyz; d["odometry_sigma_rot_deg"] = o.odometry_sigma_rot_deg;
    d["loop_sigma_xyz"] = o.loop_sigma_xyz; d["loop_sigma_rot_deg"] = o.loop_sigma_rot_deg; d["max_iterations"] = o.max_iterations;
    d["min_step"] = o.min_step;
    return d;
  };
  // the defaults (sigma: the driver's default initial_sigma) with the dict's entries over them, held to the same ranges
  auto dict2opts = [](const py::dict& d) {
    LoopClosureOptions o;
    o.sigma = mola_hip::LidarOdometry::Params().initial_sigma;
    auto num = [&](const char* k, double& v) { if (d.contains(k)) v = d[k].cast<double>(); };
    auto cnt = [&](const char* k, uint32_t& v) { if (d.contains(k)) v = d[k].cast<uint32_t>(); };
    num("min_travel", o.min_travel); num("gate_base", o.gate_base); num("gate_rate", o.gate_rate); cnt("max_place_dist", o.max_place_dist);
    cnt("top_k", o.top_k); num("min_travel_between_closures", o.min_travel_between_closures); num("submap_radius", o.submap_radius);
    num("sigma_xy", o.sigma_xy); num("sigma_yaw_deg", o.sigma_yaw_deg); num("sigma", o.sigma); num("min_quality", o.min_quality);
    num("odometry_sigma_xyz", o.odometry_sigma_xyz); num("odometry_sigma_rot_deg", o.odometry_sigma_rot_deg);
    num("loop_sigma_xyz", o.loop_sigma_xyz); num("loop_sigma_rot_deg", o.loop_sigma_rot_deg); cnt("max_iterations", o.max_iterations);
    num("min_step", o.min_step);
    o.validate();
    return o;
  };
  // the loop_closure: block of a pipeline Config as a dict (an absent block: the defaults)
  m.def("loop_closure_options", [opts2dict](const Config& c) { return opts2dict(LoopClosureOptions::FromConfig(c)); });
  // the candidate rule on host arrays: poses [K, 12], has_points [K], matches[k] = [(frame, shift, dist)] ranked as PlaceIndex.query
  // ranks them, options as a dict of loop_closure: keys, accept(i, j, shift, dist) -> bool (None: every pair is accepted).
  // -> [(i, j, shift, dist)] of the pairs handed to accept, in order
  m.def("loop_candidates", [dict2opts](py::array_t<double, py::array::c_style | py::array::forcecast> poses, const std::vector<bool>& has_points,
                                       const std::vector<std::vector<std::tuple<uint32_t, uint32_t, uint32_t>>>& matches, const py::dict& options,
                                       const py::object& accept) {
    if (poses.ndim() != 2 || poses.shape(1) != 12) throw std::runtime_error("poses must be [K, 12]");
    const size_t K = (size_t)poses.shape(0);
    if (has_points.size() != K || matches.size() != K) throw std::runtime_error("has_points and matches need one entry per pose");
    std::vector<mola_hip::LoopFrame> frames(K);
    for (size_t k = 0; k < K; k++) {
      std::copy(poses.data() + 12 * k, poses.data() + 12 * k + 12, frames[k].pose);
      frames[k].has_points = has_points[k];
      for (const auto& [f, s, d] : matches[k]) {
        if (f >= K) throw std::runtime_error("a match names frame " + std::to_string(f) + " of " + std::to_string(K));
        frames[k].matches.push_back(mola_hip::PlaceIndex::Match{f, s, d});
      }
    }
    std::function<bool(const mola_hip::LoopPair&)> verify;
    if (!accept.is_none()) verify = [&accept](const mola_hip::LoopPair& p) { return accept(p.i, p.j, p.shift, p.dist).cast<bool>(); };
    py::list out;
    for (const auto& p : mola_hip::loop_candidates(frames, dict2opts(options), verify)) out.append(py::make_tuple(p.i, p.j, p.shift, p.dist));
    return out; }, py::arg("poses"), py::arg("has_points"), py::arg("matches"), py::arg("options") = py::dict(), py::arg("accept") = py::none());
  // poses [K, 12]; loops = [(a, b, Z: 12 values, node b in node a)]; the weights and the stop as a dict of loop_closure: keys.
  // -> {poses [K, 12], cost_before, cost_after, iterations, costs}
  m.def("optimize_pose_graph", [dict2opts](py::array_t<double, py::array::c_style | py::array::forcecast> poses,
                                           const std::vector<std::tuple<uint32_t, uint32_t, std::vector<double>>>& loops, const py::dict& options) {
    if (poses.ndim() != 2 || poses.shape(1) != 12) throw std::runtime_error("poses must be [K, 12]");
    std::vector<mola_hip::PoseGraphEdge> edges;
    for (const auto& [a, b, Z] : loops) {
      if (Z.size() != 12) throw std::runtime_error("an edge's Z needs 12 values");
      mola_hip::PoseGraphEdge e;
      e.a = a; e.b = b;
      std::copy(Z.begin(), Z.end(), e.Z);
      edges.push_back(e);
    }
    const std::vector<double> in(poses.data(), poses.data() + poses.size());
    const LoopClosureOptions o = dict2opts(options);
    mola_hip::PoseGraphResult r;
    {
      py::gil_scoped_release nogil;
      r = mola_hip::optimize_pose_graph(in, edges, o);
    }
    py::array_t<double> P({poses.shape(0), (py::ssize_t)12});
    std::copy(r.poses.begin(), r.poses.end(), P.mutable_data());
    py::dict d;
    d["poses"] = P; d["cost_before"] = r.cost_before; d["cost_after"] = r.cost_after; d["iterations"] = r.iterations; d["costs"] = r.costs;
    return d; }, py::arg("poses"), py::arg("loops"), py::arg("options") = py::dict());
  // key-frames (a dict as above, or the path of a key-frame file) and the whole pipeline Config -> (corrected set as a dict, report);
  // with `output_keyframe_file` the corrected set is also written there
  m.def("close_loops", [dict2kfset, kfset2dict](const py::object& frames, const Config& pipeline, const std::string& output_keyframe_file) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    mola_hip::LoopClosureResult r;
    {
      py::gil_scoped_release nogil;
      r = mola_hip::close_loops(set, pipeline);
      if (!output_keyframe_file.empty()) molahip_host::write_keyframe_file(output_keyframe_file, r.corrected);
    }
    py::dict rep;
    py::list pairs;
    for (const auto& p : r.report.pairs) {
      py::dict d;
      d["i"] = p.i; d["j"] = p.j; d["shift"] = p.shift; d["dist"] = p.dist; d["candidates"] = p.candidates; d["ranks"] = p.ranks;
      d["quality"] = p.quality; d["iterations"] = p.iterations; d["accepted"] = p.accepted; d["Z"] = std::vector<double>(p.Z, p.Z + 12);
      pairs.append(d);
    }
    rep["pairs"] = pairs; rep["cost_before"] = r.report.cost_before; rep["cost_after"] = r.report.cost_after;
    rep["optimizer_iterations"] = r.report.optimizer_iterations; rep["seconds"] = r.report.seconds; rep["counts"] = r.report.counts;
    rep["json"] = r.report.toJson();
    return py::make_tuple(kfset2dict(r.corrected), rep); }, py::arg("frames"), py::arg("pipeline"), py::arg("output_keyframe_file") = "");
  // ---- the same while driving (mola_hip::OnlineLoopCloser)
  // the online_loop_closure: block of a pipeline Config as a dict (an absent block: the defaults)
  m.def("online_loop_closure_options", [](const Config& c) {
    const auto o = mola_hip::OnlineLoopClosureOptions::FromConfig(c);
    py::dict d;
    d["enabled"] = o.enabled; d["correct_driver"] = o.correct_driver; d["check_every_n_keyframes"] = o.check_every_n_keyframes;
    return d; });
  // the candidate rule for ONE frame i = len(poses) - 1: poses [i + 1, 12], has_points [i + 1], frame i's match list, the options,
  // state = (closed, s_closed) as the previous step returned it (None: none yet) -> ([(i, j, shift, dist)], accepted, state)
  m.def("loop_candidates_step", [dict2opts](py::array_t<double, py::array::c_style | py::array::forcecast> poses, const std::vector<bool>& has_points,
                                            const std::vector<std::tuple<uint32_t, uint32_t, uint32_t>>& matches, const py::dict& options,
                                            const py::object& state, const py::object& accept) {
    if (poses.ndim() != 2 || poses.shape(1) != 12 || poses.shape(0) < 1) throw std::runtime_error("poses must be [i + 1, 12]");
    const size_t K = (size_t)poses.shape(0);
    if (has_points.size() != K) throw std::runtime_error("has_points needs one entry per pose");
    std::vector<mola_hip::LoopFrame> frames(K);
    for (size_t k = 0; k < K; k++) {
      std::copy(poses.data() + 12 * k, poses.data() + 12 * k + 12, frames[k].pose);
      frames[k].has_points = has_points[k];
    }
    for (const auto& [f, s, d] : matches) frames[K - 1].matches.push_back(mola_hip::PlaceIndex::Match{f, s, d});  // (later frames are skipped)
    mola_hip::LoopCandidateState st;
    if (!state.is_none()) {
      const py::tuple t = state.cast<py::tuple>();
      st.closed = t[0].cast<bool>();
      st.s_closed = t[1].cast<double>();
    }
    std::function<bool(const mola_hip::LoopPair&)> verify;
    if (!accept.is_none()) verify = [&accept](const mola_hip::LoopPair& p) { return accept(p.i, p.j, p.shift, p.dist).cast<bool>(); };
    std::vector<mola_hip::LoopPair> tried;
    const bool accepted = mola_hip::loop_candidates_step(frames, mola_hip::path_lengths(frames), K - 1, dict2opts(options), st, verify, tried);
    py::list out;
    for (const auto& p : tried) out.append(py::make_tuple(p.i, p.j, p.shift, p.dist));
    return py::make_tuple(out, accepted, py::make_tuple(st.closed, st.s_closed)); },
        py::arg("poses"), py::arg("has_points"), py::arg("matches"), py::arg("options") = py::dict(), py::arg("state") = py::none(),
        py::arg("accept") = py::none());
  auto pair2dict = [](const mola_hip::LoopReport::Pair& p) {
    py::dict d;
    d["i"] = p.i; d["j"] = p.j; d["shift"] = p.shift; d["dist"] = p.dist; d["candidates"] = p.candidates; d["ranks"] = p.ranks;
    d["quality"] = p.quality; d["iterations"] = p.iterations; d["accepted"] = p.accepted; d["Z"] = std::vector<double>(p.Z, p.Z + 12);
    return d;
  };
  auto poses2array = [](const std::vector<double>& v) {
    py::array_t<double> P({(py::ssize_t)(v.size() / 12), (py::ssize_t)12});
    std::copy(v.begin(), v.end(), P.mutable_data());
    return P;
  };
  // maps: the "maps" list of a key-frame dict; push(frame): one entry of its "frames" list, the pose the RAW one
  py::class_<mola_hip::OnlineLoopCloser, std::shared_ptr<mola_hip::OnlineLoopCloser>>(m, "OnlineLoopCloser")
      .def(py::init([dict2kfset](const py::list& maps, const Config& pipeline) {
             py::dict d;
             d["maps"] = maps; d["frames"] = py::list();
             return std::make_shared<mola_hip::OnlineLoopCloser>(dict2kfset(d).maps, pipeline); }), py::arg("maps"), py::arg("pipeline"))
      .def("push", [dict2kfset, pair2dict](mola_hip::OnlineLoopCloser& c, const py::dict& frame) {
        py::dict d;
        py::list one;
        one.append(frame);
        d["maps"] = py::list(); d["frames"] = one;
        molahip_host::KeyFrameSet set = dict2kfset(d);
        mola_hip::OnlineLoopCloser::Step st;
        {
          py::gil_scoped_release nogil;
          st = c.push(std::move(set.frames[0]));
        }
        py::dict out;
        py::list pairs;
        for (const auto& p : st.pairs) pairs.append(pair2dict(p));
        out["tried"] = st.tried; out["closed"] = st.closed; out["pairs"] = pairs;
        return out; })
      .def("size", &mola_hip::OnlineLoopCloser::size)
      .def("rawPoses", [poses2array](const mola_hip::OnlineLoopCloser& c) { return poses2array(c.rawPoses()); })
      .def("correctedPoses", [poses2array](const mola_hip::OnlineLoopCloser& c) { return poses2array(c.correctedPoses()); })
      .def("loops", [](const mola_hip::OnlineLoopCloser& c) {
        py::list l;
        for (const auto& e : c.loops()) l.append(py::make_tuple(e.a, e.b, std::vector<double>(e.Z, e.Z + 12)));
        return l; })
      .def("options", [](const mola_hip::OnlineLoopCloser& c) {
        py::dict d;
        d["enabled"] = c.options().enabled; d["correct_driver"] = c.options().correct_driver;
        d["check_every_n_keyframes"] = c.options().check_every_n_keyframes;
        return d; })
      .def("rawKeyFrames", [kfset2dict](const mola_hip::OnlineLoopCloser& c) { return kfset2dict(c.rawKeyFrames()); })
      .def("report", [pair2dict](const mola_hip::OnlineLoopCloser& c) {
        const mola_hip::LoopReport& r = c.report();
        py::dict rep;
        py::list pairs;
        for (const auto& p : r.pairs) pairs.append(pair2dict(p));
        rep["pairs"] = pairs; rep["cost_before"] = r.cost_before; rep["cost_after"] = r.cost_after;
        rep["optimizer_iterations"] = r.optimizer_iterations; rep["seconds"] = r.seconds; rep["counts"] = r.counts;
        rep["json"] = r.toJson();
        return rep; });
  // ---- two sessions joined (mola_lidar_odometry_hip/SessionJoin.h)
  using mola_hip::SessionJoinOptions;
  // the session_join: block of a pipeline Config as a dict (an absent block: the defaults)
  m.def("session_join_options", [](const Config& c) {
    const SessionJoinOptions o = SessionJoinOptions::FromConfig(c);
    py::dict d;
    d["top_k"] = o.top_k; d["max_place_dist"] = o.max_place_dist; d["min_links"] = o.min_links;
    d["min_travel_between_links"] = o.min_travel_between_links; d["max_anchor_frames"] = o.max_anchor_frames;
    return d; });
  auto dict2jopts = [](const py::dict& d) {
    SessionJoinOptions o;
    auto cnt = [&](const char* k, uint32_t& v) { if (d.contains(k)) v = d[k].cast<uint32_t>(); };
    cnt("top_k", o.top_k); cnt("max_place_dist", o.max_place_dist); cnt("min_links", o.min_links); cnt("max_anchor_frames", o.max_anchor_frames);
    if (d.contains("min_travel_between_links")) o.min_travel_between_links = d["min_travel_between_links"].cast<double>();
    o.validate();
    return o;
  };
  auto frames_of = [](py::array_t<double, py::array::c_style | py::array::forcecast> poses, const std::vector<bool>& has_points, const char* what) {
    if (poses.ndim() != 2 || poses.shape(1) != 12) throw std::runtime_error(std::string(what) + ": poses must be [K, 12]");
    const size_t K = (size_t)poses.shape(0);
    if (has_points.size() != K) throw std::runtime_error(std::string(what) + ": has_points needs one entry per pose");
    std::vector<mola_hip::LoopFrame> frames(K);
    for (size_t k = 0; k < K; k++) {
      std::copy(poses.data() + 12 * k, poses.data() + 12 * k + 12, frames[k].pose);
      frames[k].has_points = has_points[k];
    }
    return frames;
  };
  // the rule's verification as a Python callable: accept(b, j, shift, dist, phase, centre [12]) -> None (rejected) or Z (12 values)
  auto join_verify = [](const py::object& accept) {
    mola_hip::JoinVerify verify;
    if (!accept.is_none())
      verify = [&accept](const mola_hip::JoinPair& p, double Z[12]) {
        const py::object r = accept(p.b, p.j, p.shift, p.dist, p.phase, std::vector<double>(p.centre, p.centre + 12));
        if (r.is_none()) return false;
        const std::vector<double> z = r.cast<std::vector<double>>();
        if (z.size() != 12) throw std::runtime_error("accept must return None or the 12 values of Z");
        std::copy(z.begin(), z.end(), Z);
        return true;
      };
    return verify;
  };
  auto jpair2tuple = [](const mola_hip::JoinPair& p) {
    return py::make_tuple(p.b, p.j, p.shift, p.dist, p.phase, std::vector<double>(p.centre, p.centre + 12));
  };
  auto jlink2tuple = [](const mola_hip::JoinLink& l) { return py::make_tuple(l.b, l.j, std::vector<double>(l.Z, l.Z + 12)); };
  // the whole candidate rule on host arrays: A's poses [KA, 12] and has_points, B's poses [KB, 12], has_points and match lists
  // (matches_b[b] = [(A frame, shift, dist)], ranked), options: session_join: keys (top_k resolved, >= 1) plus gate_base, gate_rate
  // and place_sectors.  -> (tried [(b, j, shift, dist, phase, centre)], links [(b, j, Z)])
  m.def("join_candidates", [dict2jopts, dict2opts, frames_of, join_verify, jpair2tuple, jlink2tuple](
                               py::array_t<double, py::array::c_style | py::array::forcecast> poses_a, const std::vector<bool>& has_a,
                               py::array_t<double, py::array::c_style | py::array::forcecast> poses_b, const std::vector<bool>& has_b,
                               const std::vector<std::vector<std::tuple<uint32_t, uint32_t, uint32_t>>>& matches_b, const py::dict& options,
                               const py::object& accept) {
    const std::vector<mola_hip::LoopFrame> A = frames_of(poses_a, has_a, "A");
    std::vector<mola_hip::LoopFrame> B = frames_of(poses_b, has_b, "B");
    if (matches_b.size() != B.size()) throw std::runtime_error("matches_b needs one entry per B pose");
    for (size_t b = 0; b < B.size(); b++)
      for (const auto& [f, s, d] : matches_b[b]) {
        if (f >= A.size()) throw std::runtime_error("a match names frame " + std::to_string(f) + " of " + std::to_string(A.size()));
        B[b].matches.push_back(mola_hip::PlaceIndex::Match{f, s, d});
      }
    const SessionJoinOptions o = dict2jopts(options);
    const uint32_t sectors = options.contains("place_sectors") ? options["place_sectors"].cast<uint32_t>() : 64u;
    const mola_hip::JoinCandidates c = mola_hip::join_candidates(A, B, o, o.top_k, sectors, dict2opts(options), join_verify(accept));
    py::list tried, links;
    for (const auto& p : c.tried) tried.append(jpair2tuple(p));
    for (const auto& l : c.links) links.append(jlink2tuple(l));
    return py::make_tuple(tried, links); },
        py::arg("poses_a"), py::arg("has_points_a"), py::arg("poses_b"), py::arg("has_points_b"), py::arg("matches_b"), py::arg("options") = py::dict(),
        py::arg("accept") = py::none());
  // the link rule for ONE frame b of a sweep: `matches` is frame b's list, carried = (b', j', Z') -> (tried, accepted, carried)
  m.def("join_candidates_step", [dict2jopts, dict2opts, frames_of, join_verify, jpair2tuple, jlink2tuple](
                                    py::array_t<double, py::array::c_style | py::array::forcecast> poses_a, const std::vector<bool>& has_a,
                                    py::array_t<double, py::array::c_style | py::array::forcecast> poses_b, const std::vector<bool>& has_b, size_t b,
                                    uint32_t phase, const std::vector<std::tuple<uint32_t, uint32_t, uint32_t>>& matches, const py::dict& options,
                                    const std::tuple<uint32_t, uint32_t, std::vector<double>>& carried, const py::object& accept) {
    const std::vector<mola_hip::LoopFrame> A = frames_of(poses_a, has_a, "A");
    std::vector<mola_hip::LoopFrame> B = frames_of(poses_b, has_b, "B");
    mola_hip::JoinLink link;
    link.b = std::get<0>(carried); link.j = std::get<1>(carried);
    if (b >= B.size() || link.b >= B.size() || link.j >= A.size() || std::get<2>(carried).size() != 12)
      throw std::runtime_error("join_candidates_step: b, or the carried link, names a frame that is not there");
    std::copy(std::get<2>(carried).begin(), std::get<2>(carried).end(), link.Z);
    for (const auto& [f, s, d] : matches) B[b].matches.push_back(mola_hip::PlaceIndex::Match{f, s, d});
    const SessionJoinOptions o = dict2jopts(options);
    std::vector<mola_hip::JoinPair> tried;
    const bool accepted = mola_hip::join_candidates_step(A, B, mola_hip::path_lengths(B), b, phase, o, o.top_k, dict2opts(options), link, join_verify(accept), tried);
    py::list out;
    for (const auto& p : tried) out.append(jpair2tuple(p));
    return py::make_tuple(out, accepted, jlink2tuple(link)); },
        py::arg("poses_a"), py::arg("has_points_a"), py::arg("poses_b"), py::arg("has_points_b"), py::arg("b"), py::arg("phase"), py::arg("matches"),
        py::arg("options"), py::arg("carried"), py::arg("accept") = py::none());
  // poses [K, 12], the first n_fixed fixed; chain_starts; edges = [(a, b, Z: 12 values, node b in node a)]; the weights and the stop
  // as a dict of loop_closure: keys.  -> {poses [K, 12], cost_before, cost_after, iterations, costs}
  m.def("optimize_pose_graph_anchored", [dict2opts](py::array_t<double, py::array::c_style | py::array::forcecast> poses, size_t n_fixed,
                                                    const std::vector<uint32_t>& chain_starts,
                                                    const std::vector<std::tuple<uint32_t, uint32_t, std::vector<double>>>& edges_in, const py::dict& options) {
    if (poses.ndim() != 2 || poses.shape(1) != 12) throw std::runtime_error("poses must be [K, 12]");
    std::vector<mola_hip::PoseGraphEdge> edges;
    for (const auto& [a, b, Z] : edges_in) {
      if (Z.size() != 12) throw std::runtime_error("an edge's Z needs 12 values");
      mola_hip::PoseGraphEdge e;
      e.a = a; e.b = b;
      std::copy(Z.begin(), Z.end(), e.Z);
      edges.push_back(e);
    }
    const std::vector<double> in(poses.data(), poses.data() + poses.size());
    const LoopClosureOptions o = dict2opts(options);
    mola_hip::PoseGraphResult r;
    {
      py::gil_scoped_release nogil;
      r = mola_hip::optimize_pose_graph_anchored(in, n_fixed, chain_starts, edges, o);
    }
    py::array_t<double> P({poses.shape(0), (py::ssize_t)12});
    std::copy(r.poses.begin(), r.poses.end(), P.mutable_data());
    py::dict d;
    d["poses"] = P; d["cost_before"] = r.cost_before; d["cost_after"] = r.cost_after; d["iterations"] = r.iterations; d["costs"] = r.costs;
    return d; }, py::arg("poses"), py::arg("n_fixed"), py::arg("chain_starts"), py::arg("edges"), py::arg("options") = py::dict());
  // two key-frame sets (dicts as close_loops takes them, or paths of key-frame files) and the whole pipeline Config -> (joined set as
  // a dict, is_joined, report); with `output_keyframe_file` the joined set is also written there when the sessions are joined
  m.def("join_sessions", [dict2kfset, kfset2dict](const py::object& a, const py::object& b, const Config& pipeline, const std::string& output_keyframe_file) {
    auto load = [&](const py::object& f) {
      return py::isinstance<py::str>(f) ? molahip_host::read_keyframe_file(f.cast<std::string>()) : dict2kfset(f.cast<py::dict>());
    };
    const molahip_host::KeyFrameSet A = load(a), B = load(b);
    mola_hip::SessionJoinResult r;
    {
      py::gil_scoped_release nogil;
      r = mola_hip::join_sessions(A, B, pipeline);
      if (r.is_joined && !output_keyframe_file.empty()) molahip_host::write_keyframe_file(output_keyframe_file, r.joined);
    }
    py::dict rep;
    py::list pairs;
    for (const auto& p : r.report.pairs) {
      py::dict d;
      d["i"] = p.i; d["j"] = p.j; d["phase"] = p.phase; d["shift"] = p.shift; d["dist"] = p.dist; d["candidates"] = p.candidates; d["ranks"] = p.ranks;
      d["quality"] = p.quality; d["iterations"] = p.iterations; d["accepted"] = p.accepted; d["Z"] = std::vector<double>(p.Z, p.Z + 12);
      pairs.append(d);
    }
    rep["pairs"] = pairs; rep["links_accepted"] = r.report.links_accepted; rep["joined"] = r.report.joined; rep["cost_before"] = r.report.cost_before;
    rep["cost_after"] = r.report.cost_after; rep["optimizer_iterations"] = r.report.optimizer_iterations; rep["seconds"] = r.report.seconds;
    rep["counts"] = r.report.counts; rep["json"] = r.report.toJson();
    return py::make_tuple(kfset2dict(r.joined), r.is_joined, rep); },
        py::arg("a"), py::arg("b"), py::arg("pipeline"), py::arg("output_keyframe_file") = "");
  // ---- moving objects taken out of key-frames (mola_lidar_odometry_hip/MapCleaning.h)
  using mola_hip::MapCleaningOptions;
  // `options`: a pipeline Config, or the YAML text of one (its map_cleaning: block is read; absent: the defaults)
  auto cleaning_opts = [](const py::object& options) {
    if (options.is_none()) return MapCleaningOptions::FromConfig(Config::FromYamlText(""));
    if (py::isinstance<py::str>(options)) return MapCleaningOptions::FromConfig(Config::FromYamlText(options.cast<std::string>()));
    return MapCleaningOptions::FromConfig(options.cast<const Config&>());
  };
  m.def("map_cleaning_options", [cleaning_opts](const py::object& options) {
    const MapCleaningOptions o = cleaning_opts(options);
    py::dict d;
    d["n_rings"] = o.n_rings; d["n_sectors"] = o.n_sectors; d["el_min_deg"] = o.el_min_deg; d["el_max_deg"] = o.el_max_deg;
    d["min_range"] = o.min_range; d["max_range"] = o.max_range; d["rel_margin"] = o.rel_margin;
    d["origin_x"] = o.origin[0]; d["origin_y"] = o.origin[1]; d["origin_z"] = o.origin[2];
    d["win_rings"] = o.win_rings; d["win_sectors"] = o.win_sectors; d["max_view_distance"] = o.max_view_distance;
    d["max_views_per_frame"] = o.max_views_per_frame; d["min_through_votes"] = o.min_through_votes; d["agree_weight"] = o.agree_weight;
    const mh_clean_params p = o.deviceParams();  // what the device is given: the floats of mh_clean_params
    d["device_params"] = py::make_tuple(p.n_rings, p.n_sectors, p.el_min, p.el_max, p.min_range, p.max_range, p.rel_margin,
                                        py::make_tuple(p.origin[0], p.origin[1], p.origin[2]), p.win_rings, p.win_sectors);
    return d; }, py::arg("options") = py::none());
  // poses [K, 12], has_points [K] -> the neighbour list of every frame (host rule 1)
  m.def("cleaning_neighbours", [cleaning_opts](py::array_t<double, py::array::c_style | py::array::forcecast> poses, const std::vector<bool>& has_points,
                                               const py::object& options) {
    if (poses.ndim() != 2 || poses.shape(1) != 12) throw std::runtime_error("cleaning_neighbours: poses must be [K, 12]");
    if (has_points.size() != (size_t)poses.shape(0)) throw std::runtime_error("cleaning_neighbours: has_points needs one entry per pose");
    const std::vector<double> P(poses.data(), poses.data() + poses.size());
    const std::vector<uint8_t> has(has_points.begin(), has_points.end());
    return mola_hip::cleaning_neighbours(P, has, cleaning_opts(options)); },
        py::arg("poses"), py::arg("has_points"), py::arg("options") = py::none());
  m.def("cleaning_relative_pose", [](const std::vector<double>& Ti, const std::vector<double>& Tj) {
    if (Ti.size() != 12 || Tj.size() != 12) throw std::runtime_error("a pose has 12 values");
    std::vector<double> T(12);
    mola_hip::cleaning_relative_pose(Ti.data(), Tj.data(), T.data());
    return T; });
  m.def("cleaning_removes", [cleaning_opts](py::array_t<uint32_t, py::array::c_style | py::array::forcecast> votes, const py::object& options) {
    const MapCleaningOptions o = cleaning_opts(options);
    std::vector<bool> out((size_t)votes.size());
    for (size_t k = 0; k < out.size(); k++) out[k] = mola_hip::cleaning_removes(votes.data()[k], o);
    return out; }, py::arg("votes"), py::arg("options") = py::none());
  // a key-frame set (a dict as close_loops takes it, or the path of a key-frame file) -> (cleaned set as a dict, report); with
  // `output_keyframe_file` the cleaned set is also written there
  m.def("clean_keyframes", [dict2kfset, kfset2dict, cleaning_opts](const py::object& frames, const py::object& options, const std::string& output_keyframe_file) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    const MapCleaningOptions o = cleaning_opts(options);
    mola_hip::CleaningResult r;
    {
      py::gil_scoped_release nogil;
      r = mola_hip::clean_keyframes(set, o);
      if (!output_keyframe_file.empty()) molahip_host::write_keyframe_file(output_keyframe_file, r.cleaned);
    }
    py::dict rep;
    py::list per;
    for (const auto& f : r.report.frames) per.append(py::make_tuple(f.points_in, f.points_removed, f.neighbours));
    rep["frames"] = per; rep["points_in"] = r.report.points_in; rep["points_removed"] = r.report.points_removed; rep["pairs"] = r.report.pairs;
    rep["seconds"] = r.report.seconds; rep["json"] = r.report.toJson();
    return py::make_tuple(kfset2dict(r.cleaned), rep); },
        py::arg("frames"), py::arg("options") = py::none(), py::arg("output_keyframe_file") = "");
  // ---- a navigation occupancy grid from key-frames (mola_lidar_odometry_hip/OccupancyGrid.h)
  using mola_hip::OccupancyGrid;
  using mola_hip::OccupancyGridOptions;
  // `options`: a pipeline Config, or the YAML text of one (its occupancy_grid: block is read; absent: the defaults)
  auto grid_opts = [](const py::object& options) {
    if (options.is_none()) return OccupancyGridOptions::FromConfig(Config::FromYamlText(""));
    if (py::isinstance<py::str>(options)) return OccupancyGridOptions::FromConfig(Config::FromYamlText(options.cast<std::string>()));
    return OccupancyGridOptions::FromConfig(options.cast<const Config&>());
  };
  auto grid2dict = [](const OccupancyGrid& g) {
    py::dict d;
    d["x0"] = g.x0; d["y0"] = g.y0; d["nx"] = g.nx; d["ny"] = g.ny; d["resolution"] = g.resolution;
    d["z_lo"] = g.z_lo; d["z_hi"] = g.z_hi; d["l_occ"] = g.l_occ;
    py::array_t<int32_t> mx({(py::ssize_t)(g.max_logodds.empty() ? 0 : g.ny), (py::ssize_t)g.nx});
    std::copy(g.max_logodds.begin(), g.max_logodds.end(), mx.mutable_data());
    py::array_t<int8_t> cells({(py::ssize_t)g.ny, (py::ssize_t)g.nx});
    std::copy(g.cells.begin(), g.cells.end(), cells.mutable_data());
    d["max_logodds"] = mx; d["cells"] = cells;
    d["cells_occupied"] = g.cells_occupied; d["cells_free"] = g.cells_free; d["cells_unknown"] = g.cells_unknown;
    d["frames"] = g.frames; d["points"] = g.points; d["map_cells"] = g.map_cells;
    d["seconds_insert"] = g.seconds_insert; d["seconds_project"] = g.seconds_project;
    return d;
  };
  auto dict2grid = [](const py::dict& d) {
    OccupancyGrid g;
    g.x0 = d["x0"].cast<int32_t>(); g.y0 = d["y0"].cast<int32_t>(); g.nx = d["nx"].cast<uint32_t>(); g.ny = d["ny"].cast<uint32_t>();
    g.resolution = d["resolution"].cast<double>();
    if (d.contains("l_occ")) g.l_occ = d["l_occ"].cast<int32_t>();
    if (d.contains("max_logodds") && !d.contains("cells")) {
      auto mx = d["max_logodds"].cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
      g.max_logodds.assign(mx.data(), mx.data() + mx.size());
      mola_hip::occupancy_grid_classify(g);
    } else {
      auto c = d["cells"].cast<py::array_t<int8_t, py::array::c_style | py::array::forcecast>>();
      g.cells.assign(c.data(), c.data() + c.size());
    }
    return g;
  };
  m.def("occupancy_grid_options", [grid_opts](const py::object& options) {
    const OccupancyGridOptions o = grid_opts(options);
    py::dict d;
    d["resolution"] = o.resolution; d["prob_hit"] = o.prob_hit; d["prob_miss"] = o.prob_miss; d["clamp_min"] = o.clamp_min;
    d["clamp_max"] = o.clamp_max; d["occupied_threshold"] = o.occupied_threshold; d["ray_trace_free_space"] = o.ray_trace_free_space;
    d["max_range"] = o.max_range; d["decimation"] = o.decimation; d["update_rule"] = o.update_rule; d["target_map"] = o.target_map;
    d["z_min"] = o.z_min; d["z_max"] = o.z_max; d["margin_cells"] = o.margin_cells;
    d["z_lo"] = mola_hip::occupancy_grid_z_index(o.z_min, o.resolution); d["z_hi"] = mola_hip::occupancy_grid_z_index(o.z_max, o.resolution);
    return d; }, py::arg("options") = py::none());
  m.def("occupancy_grid_z_index", &mola_hip::occupancy_grid_z_index, py::arg("z"), py::arg("resolution"));
  // int32 maxima [ny, nx] + l_occ -> (int8 cells [ny, nx], occupied, free, unknown): the trinary rule
  m.def("occupancy_grid_classify", [](py::array_t<int32_t, py::array::c_style | py::array::forcecast> max_logodds, int32_t l_occ) {
    if (max_logodds.ndim() != 2) throw std::runtime_error("occupancy_grid_classify: max_logodds must be [ny, nx]");
    OccupancyGrid g;
    g.ny = (uint32_t)max_logodds.shape(0); g.nx = (uint32_t)max_logodds.shape(1); g.l_occ = l_occ;
    g.max_logodds.assign(max_logodds.data(), max_logodds.data() + max_logodds.size());
    mola_hip::occupancy_grid_classify(g);
    py::array_t<int8_t> cells({(py::ssize_t)g.ny, (py::ssize_t)g.nx});
    std::copy(g.cells.begin(), g.cells.end(), cells.mutable_data());
    return py::make_tuple(cells, g.cells_occupied, g.cells_free, g.cells_unknown); }, py::arg("max_logodds"), py::arg("l_occ"));
  // a key-frame set (a dict, or the path of a key-frame file) -> the grid as a dict
  m.def("build_occupancy_grid", [dict2kfset, grid_opts, grid2dict](const py::object& frames, const py::object& options, uint64_t max_points_per_pass) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    const OccupancyGridOptions o = grid_opts(options);
    OccupancyGrid g;
    {
      py::gil_scoped_release nogil;
      g = mola_hip::build_occupancy_grid(set, o, nullptr, max_points_per_pass);
    }
    return grid2dict(g); }, py::arg("frames"), py::arg("options") = py::none(), py::arg("max_points_per_pass") = 0);
  m.def("write_occupancy_grid", [dict2grid](const py::dict& grid, const std::string& prefix) { mola_hip::write_occupancy_grid(dict2grid(grid), prefix); },
        py::arg("grid"), py::arg("prefix"));
  m.def("read_occupancy_grid", [grid2dict](const std::string& prefix) { return grid2dict(mola_hip::read_occupancy_grid(prefix)); }, py::arg("prefix"));
  // ---- an elevation map with a traversability cost from key-frames (mola_lidar_odometry_hip/Traversability.h)
  using mola_hip::TraversabilityMap;
  using mola_hip::TraversabilityOptions;
  // `options`: a pipeline Config, or the YAML text of one (its traversability: block is read; absent: the defaults)
  auto trav_opts = [](const py::object& options) {
    if (options.is_none()) return TraversabilityOptions::FromConfig(Config::FromYamlText(""));
    if (py::isinstance<py::str>(options)) return TraversabilityOptions::FromConfig(Config::FromYamlText(options.cast<std::string>()));
    return TraversabilityOptions::FromConfig(options.cast<const Config&>());
  };
  auto plane2array = [](const auto& v, uint32_t ny, uint32_t nx) {
    using T = typename std::decay_t<decltype(v)>::value_type;
    py::array_t<T> a({(py::ssize_t)(v.empty() ? 0 : ny), (py::ssize_t)nx});
    std::copy(v.begin(), v.end(), a.mutable_data());
    return a;
  };
  auto trav2dict = [plane2array](const TraversabilityMap& t) {
    py::dict d;
    d["x0"] = t.x0; d["y0"] = t.y0; d["nx"] = t.nx; d["ny"] = t.ny; d["resolution"] = t.resolution; d["z_quantum"] = t.z_quantum;
    d["clearance_q"] = t.clearance_q; d["step_q"] = t.step_q; d["rise_q"] = t.rise_q;
    d["min_points_per_cell"] = t.min_points_per_cell; d["min_obstacle_points"] = t.min_obstacle_points;
    d["ground"] = plane2array(t.ground, t.ny, t.nx); d["top"] = plane2array(t.top, t.ny, t.nx);
    d["count"] = plane2array(t.count, t.ny, t.nx); d["obstacle_count"] = plane2array(t.obstacle_count, t.ny, t.nx);
    d["relief1"] = plane2array(t.relief1, t.ny, t.nx); d["reliefR"] = plane2array(t.reliefR, t.ny, t.nx);
    d["cost"] = plane2array(t.cost, t.ny, t.nx); d["height"] = plane2array(t.height, t.ny, t.nx);
    d["cells_lethal"] = t.cells_lethal; d["cells_free"] = t.cells_free; d["cells_unknown"] = t.cells_unknown;
    d["frames"] = t.frames; d["points"] = t.points; d["points_counted"] = t.points_counted; d["points_left_out"] = t.points_left_out;
    d["points_outside_window"] = t.points_outside_window;
    d["seconds_bounds"] = t.seconds_bounds; d["seconds_add"] = t.seconds_add; d["seconds_mark"] = t.seconds_mark; d["seconds_relief"] = t.seconds_relief;
    return d;
  };
  m.def("traversability_options", [trav_opts](const py::object& options) {
    const TraversabilityOptions o = trav_opts(options);
    py::dict d;
    d["resolution"] = o.resolution; d["z_quantum"] = o.z_quantum; d["max_range"] = o.max_range; d["vehicle_height"] = o.vehicle_height;
    d["max_step"] = o.max_step; d["slope_radius_cells"] = o.slope_radius_cells; d["max_slope_deg"] = o.max_slope_deg;
    d["min_points_per_cell"] = o.min_points_per_cell; d["min_obstacle_points"] = o.min_obstacle_points; d["target_map"] = o.target_map;
    d["margin_cells"] = o.margin_cells;
    d["clearance_q"] = o.clearanceQ(); d["step_q"] = o.stepQ(); d["rise_q"] = o.riseQ();
    return d; }, py::arg("options") = py::none());
  // the host rule on given planes [ny, nx] -> (uint8 cost, float32 height, lethal, free, unknown)
  m.def("traversability_classify", [plane2array](py::array_t<int32_t, py::array::c_style | py::array::forcecast> ground,
                                                 py::array_t<uint32_t, py::array::c_style | py::array::forcecast> count,
                                                 py::array_t<uint32_t, py::array::c_style | py::array::forcecast> obstacle_count,
                                                 py::array_t<int32_t, py::array::c_style | py::array::forcecast> relief1,
                                                 py::array_t<int32_t, py::array::c_style | py::array::forcecast> reliefR, int32_t step_q, int32_t rise_q,
                                                 uint32_t min_points_per_cell, uint32_t min_obstacle_points, double z_quantum) {
    if (count.ndim() != 2) throw std::runtime_error("traversability_classify: the planes must be [ny, nx]");
    TraversabilityMap t;
    t.ny = (uint32_t)count.shape(0); t.nx = (uint32_t)count.shape(1);
    t.step_q = step_q; t.rise_q = rise_q; t.min_points_per_cell = min_points_per_cell; t.min_obstacle_points = min_obstacle_points;
    t.z_quantum = z_quantum;
    t.ground.assign(ground.data(), ground.data() + ground.size());
    t.count.assign(count.data(), count.data() + count.size());
    t.obstacle_count.assign(obstacle_count.data(), obstacle_count.data() + obstacle_count.size());
    t.relief1.assign(relief1.data(), relief1.data() + relief1.size());
    t.reliefR.assign(reliefR.data(), reliefR.data() + reliefR.size());
    mola_hip::traversability_classify(t);
    return py::make_tuple(plane2array(t.cost, t.ny, t.nx), plane2array(t.height, t.ny, t.nx), t.cells_lethal, t.cells_free, t.cells_unknown); },
        py::arg("ground"), py::arg("count"), py::arg("obstacle_count"), py::arg("relief1"), py::arg("reliefR"), py::arg("step_q"), py::arg("rise_q"),
        py::arg("min_points_per_cell") = 2, py::arg("min_obstacle_points") = 2, py::arg("z_quantum") = 0.01);
  // a key-frame set (a dict, or the path of a key-frame file) -> the map as a dict
  m.def("build_traversability_map", [dict2kfset, trav_opts, trav2dict](const py::object& frames, const py::object& options, uint64_t max_points_per_pass) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    const TraversabilityOptions o = trav_opts(options);
    TraversabilityMap t;
    {
      py::gil_scoped_release nogil;
      t = mola_hip::build_traversability_map(set, o, nullptr, max_points_per_pass);
    }
    return trav2dict(t); }, py::arg("frames"), py::arg("options") = py::none(), py::arg("max_points_per_pass") = 0);
  m.def("write_traversability_map", [](const py::dict& d, const std::string& prefix) {
    TraversabilityMap t;
    t.x0 = d["x0"].cast<int32_t>(); t.y0 = d["y0"].cast<int32_t>(); t.nx = d["nx"].cast<uint32_t>(); t.ny = d["ny"].cast<uint32_t>();
    t.resolution = d["resolution"].cast<double>(); t.z_quantum = d["z_quantum"].cast<double>();
    auto c = d["cost"].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
    auto h = d["height"].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
    t.cost.assign(c.data(), c.data() + c.size());
    t.height.assign(h.data(), h.data() + h.size());
    mola_hip::write_traversability_map(t, prefix); }, py::arg("map"), py::arg("prefix"));
  m.def("read_traversability_map", [trav2dict](const std::string& prefix) { return trav2dict(mola_hip::read_traversability_map(prefix)); },
        py::arg("prefix"));
  // ---- an inflated costmap with the reachable region (mola_lidar_odometry_hip/NavCostmap.h)
  using mola_hip::CostmapBase;
  using mola_hip::NavCostmap;
  using mola_hip::NavCostmapOptions;
  using mola_hip::Pose12;
  // `options`: a pipeline Config, or the YAML text of one (its costmap: block is read; absent: the defaults)
  auto nav_cfg = [](const py::object& options) {
    if (options.is_none()) return Config::FromYamlText("");
    if (py::isinstance<py::str>(options)) return Config::FromYamlText(options.cast<std::string>());
    return options.cast<Config>();
  };
  // a source map as a dict: a traversability map (`cost` uint8) or an occupancy grid (`cells` int8), with x0, y0, nx, ny, resolution
  auto dict2base = [dict2grid](const py::dict& d) {
    if (d.contains("cells")) return mola_hip::costmap_base(dict2grid(d));
    TraversabilityMap t;
    t.x0 = d["x0"].cast<int32_t>(); t.y0 = d["y0"].cast<int32_t>(); t.nx = d["nx"].cast<uint32_t>(); t.ny = d["ny"].cast<uint32_t>();
    t.resolution = d["resolution"].cast<double>();
    auto c = d["cost"].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
    t.cost.assign(c.data(), c.data() + c.size());
    return mola_hip::costmap_base(t);
  };
  auto to_poses = [](const std::vector<std::vector<double>>& poses) {
    std::vector<Pose12> out(poses.size());
    for (size_t k = 0; k < poses.size(); k++) {
      if (poses[k].size() != 12) throw std::runtime_error("a pose has 12 values");
      std::copy(poses[k].begin(), poses[k].end(), out[k].begin());
    }
    return out;
  };
  auto nav2dict = [plane2array](const NavCostmap& c) {
    py::dict d;
    d["x0"] = c.x0; d["y0"] = c.y0; d["nx"] = c.nx; d["ny"] = c.ny; d["resolution"] = c.resolution;
    d["inscribed_radius"] = c.inscribed_radius; d["inflation_radius"] = c.inflation_radius; d["max_cells"] = c.max_cells;
    d["unknown_is_obstacle"] = c.unknown_is_obstacle;
    d["d2"] = plane2array(c.d2, c.ny, c.nx); d["cost"] = plane2array(c.cost, c.ny, c.nx); d["reach"] = plane2array(c.reach, c.ny, c.nx);
    d["cells_lethal"] = c.cells_lethal; d["cells_inscribed"] = c.cells_inscribed; d["cells_inflated"] = c.cells_inflated;
    d["cells_free"] = c.cells_free; d["cells_unknown"] = c.cells_unknown; d["cells_reached"] = c.cells_reached;
    d["cells_unreachable_free"] = c.cells_unreachable_free;
    d["keyframe_d2"] = std::vector<uint32_t>(c.keyframe_d2.begin(), c.keyframe_d2.end());
    d["keyframe_cost"] = std::vector<uint32_t>(c.keyframe_cost.begin(), c.keyframe_cost.end());
    d["keyframe_reached"] = std::vector<uint32_t>(c.keyframe_reached.begin(), c.keyframe_reached.end());
    d["trajectory_min_clearance_m"] = c.trajectory_min_clearance_m; d["keyframes_blocked"] = c.keyframes_blocked;
    d["seeds"] = c.seeds; d["seeds_blocked"] = c.seeds_blocked; d["seeds_outside"] = c.seeds_outside; d["sweeps"] = c.sweeps;
    d["seconds_source"] = c.seconds_source; d["seconds_inflate"] = c.seconds_inflate; d["seconds_reach"] = c.seconds_reach;
    return d;
  };
  auto dict2nav = [](const py::dict& d) {
    NavCostmap c;
    c.x0 = d["x0"].cast<int32_t>(); c.y0 = d["y0"].cast<int32_t>(); c.nx = d["nx"].cast<uint32_t>(); c.ny = d["ny"].cast<uint32_t>();
    c.resolution = d["resolution"].cast<double>();
    c.inscribed_radius = d["inscribed_radius"].cast<double>(); c.inflation_radius = d["inflation_radius"].cast<double>();
    auto cost = d["cost"].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
    auto reach = d["reach"].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
    c.cost.assign(cost.data(), cost.data() + cost.size());
    c.reach.assign(reach.data(), reach.data() + reach.size());
    if (d.contains("d2")) {
      auto d2 = d["d2"].cast<py::array_t<uint16_t, py::array::c_style | py::array::forcecast>>();
      c.d2.assign(d2.data(), d2.data() + d2.size());
    }
    return c;
  };
  m.def("costmap_options", [nav_cfg](const py::object& options) {
    const NavCostmapOptions o = NavCostmapOptions::FromConfig(nav_cfg(options));
    py::dict d;
    d["source"] = o.source; d["inscribed_radius"] = o.inscribed_radius; d["inflation_radius"] = o.inflation_radius;
    d["cost_scaling"] = o.cost_scaling; d["unknown_is_obstacle"] = o.unknown_is_obstacle; d["reach_from"] = o.reach_from;
    return d; }, py::arg("options") = py::none());
  // rule 2 -> uint8 [R * R + 1]
  m.def("inflation_table", [nav_cfg](const py::object& options, double resolution) {
    const std::vector<uint8_t> t = mola_hip::inflation_table(NavCostmapOptions::FromConfig(nav_cfg(options)), resolution);
    py::array_t<uint8_t> a((py::ssize_t)t.size());
    std::copy(t.begin(), t.end(), a.mutable_data());
    return a; }, py::arg("options") = py::none(), py::arg("resolution") = 0.2);
  // rule 1 -> uint8 [ny, nx]
  m.def("costmap_base", [dict2base, plane2array](const py::dict& map) {
    const CostmapBase b = dict2base(map);
    return plane2array(b.bytes, b.ny, b.nx); }, py::arg("map"));
  // rule 3 -> (column, row) pairs relative to the window of `map`
  m.def("costmap_seeds", [dict2base, to_poses](const py::dict& map, const std::vector<std::vector<double>>& poses, const std::string& reach_from) {
    return mola_hip::costmap_seeds(dict2base(map), to_poses(poses), reach_from); }, py::arg("map"), py::arg("poses"), py::arg("reach_from") = "keyframes");
  // rule 4 on given planes (a dict with the window, the resolution, the radii, cost, reach and optionally d2) -> the costmap dict
  m.def("costmap_summarise", [dict2nav, nav2dict, to_poses](const py::dict& map, const std::vector<std::vector<double>>& poses) {
    NavCostmap c = dict2nav(map);
    mola_hip::costmap_summarise(c, to_poses(poses));
    return nav2dict(c); }, py::arg("map"), py::arg("poses"));
  m.def("build_costmap", [dict2base, nav_cfg, to_poses, nav2dict](const py::dict& map, const std::vector<std::vector<double>>& poses, const py::object& options) {
    const CostmapBase b = dict2base(map);
    const NavCostmapOptions o = NavCostmapOptions::FromConfig(nav_cfg(options));
    const std::vector<Pose12> p = to_poses(poses);
    NavCostmap c;
    {
      py::gil_scoped_release nogil;
      c = mola_hip::build_costmap(b, p, o);
    }
    return nav2dict(c); }, py::arg("map"), py::arg("poses"), py::arg("options") = py::none());
  // a key-frame set (a dict, or the path of a key-frame file) -> the costmap as a dict
  m.def("build_costmap_from_keyframes", [dict2kfset, nav_cfg, nav2dict](const py::object& frames, const py::object& options) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    const Config cfg = nav_cfg(options);
    NavCostmap c;
    {
      py::gil_scoped_release nogil;
      c = mola_hip::build_costmap_from_keyframes(set, cfg);
    }
    return nav2dict(c); }, py::arg("frames"), py::arg("options") = py::none());
  m.def("write_costmap", [dict2nav](const py::dict& d, const std::string& prefix) { mola_hip::write_costmap(dict2nav(d), prefix); }, py::arg("map"),
        py::arg("prefix"));
  m.def("read_costmap", [nav2dict](const std::string& prefix) { return nav2dict(mola_hip::read_costmap(prefix)); }, py::arg("prefix"));
  // ---- a route over a costmap (mola_lidar_odometry_hip/RoutePlan.h)
  using mola_hip::RouteOptions;
  using mola_hip::RoutePlan;
  auto route2dict = [](const RoutePlan& r, uint32_t nx, uint32_t ny) {
    py::dict d;
    d["status"] = r.status;
    d["start_cell"] = py::make_tuple(r.start_col, r.start_row); d["goal_cell"] = py::make_tuple(r.goal_col, r.goal_row);
    py::array_t<int32_t> cells({(py::ssize_t)(r.cells.size() / 2), (py::ssize_t)2});
    std::copy(r.cells.begin(), r.cells.end(), cells.mutable_data());
    py::array_t<double> xy({(py::ssize_t)(r.xy.size() / 2), (py::ssize_t)2});
    std::copy(r.xy.begin(), r.xy.end(), xy.mutable_data());
    d["cells"] = cells; d["xy"] = xy;
    d["length_m"] = r.length_m; d["cost_to_go"] = r.cost_to_go; d["max_cost"] = r.max_cost; d["min_clearance_m"] = r.min_clearance_m;
    if (r.field.empty()) d["field"] = py::none();
    else {
      py::array_t<uint32_t> f({(py::ssize_t)ny, (py::ssize_t)nx});
      std::copy(r.field.begin(), r.field.end(), f.mutable_data());
      d["field"] = f;
    }
    d["sweeps"] = r.sweeps; d["tile_runs"] = r.tile_runs; d["cells_with_field"] = r.cells_with_field;
    d["seconds_field"] = r.seconds_field; d["seconds_trace"] = r.seconds_trace;
    return d;
  };
  auto dict2route = [](const py::dict& d) {
    RoutePlan r;
    auto cells = d["cells"].cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
    r.cells.assign(cells.data(), cells.data() + cells.size());
    if (d.contains("xy")) {
      auto xy = d["xy"].cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
      r.xy.assign(xy.data(), xy.data() + xy.size());
    }
    return r;
  };
  m.def("route_options", [nav_cfg](const py::object& options) {
    const RouteOptions o = RouteOptions::FromConfig(nav_cfg(options));
    py::dict d;
    d["start_x"] = o.start_x; d["start_y"] = o.start_y; d["goal_x"] = o.goal_x; d["goal_y"] = o.goal_y;
    d["start_keyframe"] = o.start_keyframe; d["goal_keyframe"] = o.goal_keyframe; d["neutral_price"] = o.neutral_price;
    d["cost_factor"] = o.cost_factor; d["max_route_cells"] = o.max_route_cells;
    return d; }, py::arg("options") = py::none());
  // rule 1 -> uint16 [253]; with n_cells > 0 the wrap-around bound for a window of that many cells is checked as well
  m.def("route_price_table", [nav_cfg](const py::object& options, uint64_t n_cells) {
    const std::vector<uint16_t> t = mola_hip::route_price_table(RouteOptions::FromConfig(nav_cfg(options)));
    if (n_cells) mola_hip::route_check_window(t, n_cells);
    py::array_t<uint16_t> a((py::ssize_t)t.size());
    std::copy(t.begin(), t.end(), a.mutable_data());
    return a; }, py::arg("options") = py::none(), py::arg("n_cells") = 0);
  // rule 2 -> (column, row), (-1, -1) for a point without a cell in the window of `map`
  m.def("route_cell", [dict2nav](const py::dict& map, double x, double y) {
    int32_t col, row;
    (void)mola_hip::route_cell(dict2nav(map), x, y, col, row);
    return py::make_tuple(col, row); }, py::arg("map"), py::arg("x"), py::arg("y"));
  // rule 3 on given cells (int32 [n, 2]) -> the route dict
  m.def("route_summarise", [dict2nav, dict2route, route2dict](const py::dict& route, const py::dict& map) {
    const NavCostmap c = dict2nav(map);
    RoutePlan r = dict2route(route);
    mola_hip::route_summarise(r, c);
    return route2dict(r, c.nx, c.ny); }, py::arg("route"), py::arg("map"));
  m.def("plan_route", [dict2nav, nav_cfg, route2dict](const py::dict& map, const py::object& options) {
    const NavCostmap c = dict2nav(map);
    const RouteOptions o = RouteOptions::FromConfig(nav_cfg(options));
    RoutePlan r;
    {
      py::gil_scoped_release nogil;
      r = mola_hip::plan_route(c, o);
    }
    return route2dict(r, c.nx, c.ny); }, py::arg("map"), py::arg("options") = py::none());
  // a key-frame set (a dict, or the path of a key-frame file) -> the route dict, with the costmap it was planned on under "costmap"
  m.def("plan_route_from_keyframes", [dict2kfset, nav_cfg, nav2dict, route2dict](const py::object& frames, const py::object& options) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    const Config cfg = nav_cfg(options);
    mola_hip::RouteFromKeyframes out;
    {
      py::gil_scoped_release nogil;
      out = mola_hip::plan_route_from_keyframes(set, cfg);
    }
    py::dict d = route2dict(out.route, out.costmap.nx, out.costmap.ny);
    d["costmap"] = nav2dict(out.costmap);
    return d; }, py::arg("frames"), py::arg("options") = py::none());
  m.def("write_route", [dict2nav, dict2route](const py::dict& route, const py::dict& map, const std::string& prefix) {
    const NavCostmap c = dict2nav(map);
    RoutePlan r = dict2route(route);
    if (r.xy.empty()) mola_hip::route_summarise(r, c);
    mola_hip::write_route(r, c, prefix); }, py::arg("route"), py::arg("map"), py::arg("prefix"));
  // ---- routes that follow a changing costmap (mola_lidar_odometry_hip/Replan.h)
  using mola_hip::CellRect;
  using mola_hip::ReplanEvent;
  auto rect2py = [](const CellRect& r) -> py::object {
    if (r.empty) return py::none();
    return py::make_tuple(r.col0, r.row0, r.w, r.h);
  };
  auto update2dict = [rect2py](const mola_hip::ReplanUpdate& u) {
    py::dict d;
    d["rect"] = rect2py(u.rect); d["grown"] = rect2py(u.grown);
    d["cells_changed"] = u.info.n_cells_changed; d["cells_repriced"] = u.info.n_cells_repriced; d["withdrawn"] = u.info.n_withdrawn;
    d["withdraw_sweeps"] = u.info.n_withdraw_sweeps; d["relax_sweeps"] = u.info.n_relax_sweeps;
    d["tile_runs_withdraw"] = u.info.n_tile_runs_withdraw; d["tile_runs_relax"] = u.info.n_tile_runs_relax; d["updates"] = u.info.n_updates;
    d["seconds_inflate"] = u.seconds_inflate; d["seconds_update"] = u.seconds_update;
    return d;
  };
  // rule 8 -> a list of dicts (verb, numbers, line)
  m.def("replan_parse_events", [](const std::string& text) {
    py::list out;
    for (const ReplanEvent& e : mola_hip::parse_replan_events(text)) {
      py::dict d;
      d["verb"] = std::string(e.verbName());
      d["numbers"] = std::vector<double>(e.v, e.v + (e.verb == ReplanEvent::kAt ? 2 : 4));
      d["line"] = e.line;
      out.append(d);
    }
    return out; }, py::arg("text"));
  // rule 9 on a window dict (x0, y0, nx, ny, resolution) -> (col0, row0, w, h) or None
  m.def("replan_metre_rect", [rect2py](const py::dict& win, double xa, double ya, double xb, double yb) {
    NavCostmap c;
    c.x0 = win["x0"].cast<int32_t>(); c.y0 = win["y0"].cast<int32_t>(); c.nx = win["nx"].cast<uint32_t>(); c.ny = win["ny"].cast<uint32_t>();
    c.resolution = win["resolution"].cast<double>();
    return rect2py(mola_hip::replan_metre_rect(c, xa, ya, xb, yb)); }, py::arg("window"), py::arg("xa"), py::arg("ya"), py::arg("xb"), py::arg("yb"));
  // rule 5 -> (col0, row0, w, h)
  m.def("replan_grown_rect", [rect2py](uint32_t col0, uint32_t row0, uint32_t w, uint32_t h, uint32_t max_cells, uint32_t nx, uint32_t ny) {
    CellRect r;
    r.empty = false;
    r.col0 = col0; r.row0 = row0; r.w = w; r.h = h;
    return rect2py(mola_hip::replan_grown_rect(r, max_cells, nx, ny)); });
  // a planner that lives across updates: RoutePlanner(map, poses, options) with the source map dict of build_costmap and a pipeline
  // text with costmap: and route: blocks (goal_x / goal_y needed)
  py::class_<mola_hip::RoutePlanner>(m, "RoutePlanner")
      .def(py::init([dict2base, nav_cfg, to_poses](const py::dict& map, const std::vector<std::vector<double>>& poses, const py::object& options) {
             const Config cfg = nav_cfg(options);
             return std::make_unique<mola_hip::RoutePlanner>(dict2base(map), to_poses(poses), NavCostmapOptions::FromConfig(cfg), RouteOptions::FromConfig(cfg));
           }),
           py::arg("map"), py::arg("poses"), py::arg("options") = py::none())
      .def("update", [update2dict](mola_hip::RoutePlanner& p, uint32_t col0, uint32_t row0, const py::array_t<uint8_t, py::array::c_style | py::array::forcecast>& bytes) {
             if (bytes.ndim() != 2) throw std::runtime_error("RoutePlanner.update: bytes is uint8 [h, w]");
             mola_hip::ReplanUpdate u;
             const uint32_t h = (uint32_t)bytes.shape(0), w = (uint32_t)bytes.shape(1);
             const uint8_t* data = bytes.data();
             {
               py::gil_scoped_release nogil;
               u = p.update(col0, row0, w, h, data);
             }
             return update2dict(u); }, py::arg("col0"), py::arg("row0"), py::arg("bytes"))
      .def("route_from", [route2dict](mola_hip::RoutePlanner& p, double x, double y) {
             RoutePlan r;
             {
               py::gil_scoped_release nogil;
               r = p.routeFrom(x, y);
             }
             return route2dict(r, p.base().nx, p.base().ny); }, py::arg("x"), py::arg("y"))
      .def("costmap", [nav2dict](mola_hip::RoutePlanner& p) { return nav2dict(p.costmap()); })
      .def("base", [plane2array](mola_hip::RoutePlanner& p) { return plane2array(p.base().bytes, p.base().ny, p.base().nx); })
      .def_property_readonly("max_cells", &mola_hip::RoutePlanner::maxCells);
  // a key-frame set (a dict, or the path of a key-frame file), a pipeline and an events text -> a dict: "events" (one dict per event),
  // "routes" (one route dict per `at`, with the costmap it was traced on under "costmap"), "costmap" (after the last event),
  // "rects_outside", "summaries" (the command line's one line per event)
  m.def("replan_route_from_keyframes", [dict2kfset, nav_cfg, nav2dict, route2dict, update2dict](const py::object& frames, const py::object& options,
                                                                                              const std::string& events) {
    const molahip_host::KeyFrameSet set = py::isinstance<py::str>(frames) ? molahip_host::read_keyframe_file(frames.cast<std::string>())
                                                                         : dict2kfset(frames.cast<py::dict>());
    const Config cfg = nav_cfg(options);
    const std::vector<ReplanEvent> ev = mola_hip::parse_replan_events(events);
    mola_hip::ReplanRun run;
    {
      py::gil_scoped_release nogil;
      run = mola_hip::replan_route_from_keyframes(set, cfg, ev);
    }
    py::dict out;
    py::list evs, routes, lines;
    for (size_t k = 0; k < run.events.size(); k++) {
      const mola_hip::ReplanEventResult& e = run.events[k];
      py::dict d = e.event.verb == ReplanEvent::kAt ? py::dict() : update2dict(e.update);
      d["verb"] = std::string(e.event.verbName()); d["line"] = e.event.line; d["route"] = e.route;
      evs.append(d);
      lines.append(mola_hip::replan_event_summary(run, k));
    }
    for (size_t k = 0; k < run.routes.size(); k++) {
      py::dict d = route2dict(run.routes[k], run.costmap.nx, run.costmap.ny);
      d["costmap"] = nav2dict(run.route_costmaps[k]);
      routes.append(d);
    }
    out["events"] = evs; out["routes"] = routes; out["summaries"] = lines;
    out["costmap"] = nav2dict(run.costmap); out["rects_outside"] = run.rects_outside;
    return out; }, py::arg("frames"), py::arg("options"), py::arg("events"));
  // the pose rules of the driver's online loop closure and the motion model's rebase, on 12-value poses
  auto to_pose = [](const std::vector<double>& T) {
    if (T.size() != 12) throw std::runtime_error("a pose has 12 values");
    CPose3D p;
    std::copy(T.begin(), T.end(), p.T);
    return p;
  };
  auto from_pose = [](const CPose3D& p) { return std::vector<double>(p.T, p.T + 12); };
  m.def("loop_raw_pose", [to_pose, from_pose](const std::vector<double>& raw_prev, const std::vector<double>& P, const std::vector<double>& S_prev) {
    return from_pose(mola_hip::loop_raw_pose(to_pose(raw_prev), to_pose(P), to_pose(S_prev))); });
  m.def("loop_correction", [to_pose, from_pose](const std::vector<double>& C, const std::vector<double>& P) {
    return from_pose(mola_hip::loop_correction(to_pose(C), to_pose(P))); });
  m.def("trajectory_anchor", [to_pose, from_pose](const std::vector<double>& P, const std::vector<double>& S) {
    return from_pose(mola_hip::trajectory_anchor(to_pose(P), to_pose(S))); });
  m.def("trajectory_corrected", [to_pose, from_pose](const std::vector<double>& C, const std::vector<double>& rel) {
    return from_pose(mola_hip::trajectory_corrected(to_pose(C), to_pose(rel))); });
  // the constant-velocity motion model: fuse_pose(t, pose), estimated_navstate(t) -> (pose, twist [6]) or None, rebase(delta)
  py::class_<mola_hip::NavStateFuse>(m, "NavStateFuse")
      .def(py::init<>())
      .def("fuse_pose", [to_pose](mola_hip::NavStateFuse& n, double t, const std::vector<double>& pose) { n.fuse_pose(t, to_pose(pose)); })
      .def("estimated_navstate", [from_pose](const mola_hip::NavStateFuse& n, double t) -> py::object {
        const auto ns = n.estimated_navstate(t);
        if (!ns) return py::none();
        const mola_hip::Twist& w = ns->twist;
        return py::make_tuple(from_pose(ns->pose.mean), std::vector<double>{w.vx, w.vy, w.vz, w.wx, w.wy, w.wz}); })
      .def("rebase", [to_pose](mola_hip::NavStateFuse& n, const std::vector<double>& delta) { n.rebase(to_pose(delta)); });
  m.def("icp_pipeline_from_yaml", [](const Config& c) { auto t = icp_pipeline_from_yaml(c); return py::make_tuple(std::get<0>(t), std::get<1>(t)); });
}
