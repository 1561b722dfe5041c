#!/bin/bash
# builds tools/replan_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer -- the host code under test
# (route_replan.cpp, route_plan.cpp, nav_costmap.cpp, occupancy_grid.cpp, traversability.cpp, keyframe_file.cpp, map_files.cpp, config.cpp) compiled into
# the program with them -- and runs it.  No device is needed.  The libraries must be built (the program links the rest of the host layer from
# libmolahip_host.so).
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
H=$ROOT/mola_lidar_odometry_amd/host
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread -Wall -Wextra \
    -I"$H/include" -I"$ROOT/include" "$ROOT/tools/replan_host_check.cpp" "$H/src/route_replan.cpp" "$H/src/route_plan.cpp" "$H/src/nav_costmap.cpp" \
    "$H/src/occupancy_grid.cpp" "$H/src/traversability.cpp" "$H/src/keyframe_file.cpp" "$H/src/map_files.cpp" "$H/src/config.cpp" \
    -L"$ROOT/mola_lidar_odometry_amd" -lmolahip_host -lmolahip -Wl,-rpath,"$ROOT/mola_lidar_odometry_amd" -o "$OUT/replan_host_check"
"$OUT/replan_host_check" "$OUT"
