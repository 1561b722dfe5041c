#!/bin/bash
# debug library with wall_clock64 phase stamps and the flat matcher's counters (-DMH_DEBUG_PHASES) -> tools/libmolahip_dbg.so
# (objects under /tmp)
set -e
REPO=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
cd $REPO/mola_lidar_odometry_amd/csrc
mkdir -p /tmp/mh_dbg
pids=()
for f in mh_api mh_map mh_icp mh_preprocess mh_occmap mh_query mh_place; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -Wno-unused-function --offload-arch=gfx950 -I../../include -DMH_DEBUG_PHASES $EXTRA_DBG_FLAGS -c $f.hip -o /tmp/mh_dbg/$f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $REPO/tools/libmolahip_dbg.so /tmp/mh_dbg/*.o
