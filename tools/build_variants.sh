#!/bin/bash
# An A/B library of the product sources with other compile-time knobs (the `#ifndef KNOB` defaults in csrc/: MH_FLAT_W, MH_FLAT_PROBES,
# MH_FLAT_CHUNKS, MH_FLAT_WAVES, MH_LW_*, MH_ACC_PPT, MH_QUAD_W, ...) -> tools/variants/libmolahip_$NAME.so:
#   EXTRA_FLAGS="-DMH_FLAT_W=6" NAME=w6 tools/build_variants.sh
# Tests and tools pick it with MOLAHIP_LIB_PATH=<file> (+ LD_LIBRARY_PATH of a directory that holds it as libmolahip.so for the C++
# host layer).  (The tile / wave / sorted-scan matchers this script used to add were removed: their sources are in the history, their
# measurements in profiles/r02_tile_matcher.md and r04_match_kernel.md.)
set -e
REPO=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
NAME=${NAME:-ab}
OBJ=/tmp/mh_var_$NAME
cd $REPO/mola_lidar_odometry_amd/csrc
mkdir -p $REPO/tools/variants $OBJ
pids=()
for f in mh_api mh_map mh_icp mh_preprocess mh_occmap mh_query mh_place; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -Wno-unused-function --offload-arch=gfx950 -I../../include \
    $EXTRA_FLAGS -c $f.hip -o $OBJ/$f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done  # (set -e: a unit that does not compile ends the script, its errors on the terminal)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $REPO/tools/variants/libmolahip_$NAME.so $OBJ/*.o
ls -la $REPO/tools/variants/libmolahip_$NAME.so
