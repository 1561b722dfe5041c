"""The eighth public header, include/molahip_plan.h, the parts that need no device: what it declares is what the library exports and
what mola_lidar_odometry_amd/capi_plan.py binds; the structure's size and offsets against a compiled C snippet; the seven older
headers' versions; the tile constants; the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_plan.h")

NAMES = ["mh_plan_api_version", "mh_plan_create", "mh_plan_destroy", "mh_plan_download", "mh_plan_field", "mh_plan_get_info",
         "mh_plan_set_cost", "mh_plan_set_cost_from_nav", "mh_plan_trace"]
OLDER = ("molahip.h", "molahip_clean.h", "molahip_live.h", "molahip_occgrid.h", "molahip_motion.h", "molahip_elevation.h", "molahip_nav.h")


@pytest.fixture(scope="module")
def cp():
    from mola_lidar_odometry_amd import capi_plan
    return capi_plan


def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_eighth_header_is_declared_exported_and_bound(cp):
    from mola_lidar_odometry_amd import capi, capi_clean, capi_elevation, capi_live, capi_motion, capi_nav, capi_occgrid
    fns = declared()
    assert fns == sorted(cp._SIGNATURES) == NAMES
    assert all(f.startswith("mh_plan_") for f in fns)
    for other in (capi, capi_clean, capi_live, capi_occgrid, capi_motion, capi_elevation, capi_nav):   # nothing of it is in the other seven tables
        assert not set(fns) & set(other._SIGNATURES)
    L = cp.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_plan_api_version()) == cp.PLAN_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7                                      # the first header's version is untouched
    for other, fn in ((capi_clean, "mh_clean_api_version"), (capi_live, "mh_live_api_version"), (capi_occgrid, "mh_occgrid_api_version"),
                      (capi_motion, "mh_motion_api_version"), (capi_elevation, "mh_elev_api_version"), (capi_nav, "mh_nav_api_version")):
        assert int(getattr(other.lib(), fn)()) == 1, fn                      # ... and so are the six later ones'
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    assert {s for s in exported if s.startswith("mh_plan")} == set(fns)      # nothing of it is exported undeclared
    assert len({s for s in exported if s.startswith("mh_nav")}) == 8         # the seventh header's surface has not grown
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):               # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d
    for name in OLDER:
        assert "mh_plan" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_the_header_compiles_as_c_and_the_layout_is_the_mirror_s(cp, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip_plan.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mh_plan_info), offsetof(mh_plan_info, nx), offsetof(mh_plan_info, ny),
    offsetof(mh_plan_info, has_cost), offsetof(mh_plan_info, has_field), offsetof(mh_plan_info, passable_below), offsetof(mh_plan_info, n_sweeps),
    offsetof(mh_plan_info, max_field), offsetof(mh_plan_info, reserved_), offsetof(mh_plan_info, n_reached), offsetof(mh_plan_info, n_goals_blocked),
    offsetof(mh_plan_info, n_goals_outside), offsetof(mh_plan_info, n_tile_runs));
  printf("%d %lu %lu %d %d %d %d %d %d\n", MH_PLAN_API_VERSION, (unsigned long)MH_PLAN_UNREACHED, (unsigned long)MH_PLAN_TRUNCATED, MH_PLAN_TILE_X,
    MH_PLAN_TILE_Y, MH_PLAN_STEP_ORTHOGONAL, MH_PLAN_STEP_DIAGONAL, MH_ABI_VERSION, MH_NAV_API_VERSION);
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    I = cp.PlanInfo
    assert [int(v) for v in a.split()] == [C.sizeof(I), I.nx.offset, I.ny.offset, I.has_cost.offset, I.has_field.offset, I.passable_below.offset,
                                           I.n_sweeps.offset, I.max_field.offset, I.reserved_.offset, I.n_reached.offset,
                                           I.n_goals_blocked.offset, I.n_goals_outside.offset, I.n_tile_runs.offset] \
        == [64, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56]
    assert [int(v) for v in b.split()] == [1, cp.UNREACHED, cp.TRUNCATED, cp.TILE_X, cp.TILE_Y, cp.STEP_ORTHOGONAL, cp.STEP_DIAGONAL, 7, 1] \
        == [1, 0xFFFFFFFF, 0xFFFFFFFF, 64, 16, 5, 7, 7, 1]


def test_the_kernel_constants_are_the_header_s(cp):
    """the tile the header names is the one the kernels are built with, and the step lengths are the rule's"""
    k = open(os.path.join(ROOT, "mola_lidar_odometry_amd", "csrc", "mh_k_plan.h")).read()
    assert re.search(r"kPlanCells = %du" % (cp.TILE_X * cp.TILE_Y), k)
    assert re.search(r"kStepOrth = %du, kStepDiag = %du" % (cp.STEP_ORTHOGONAL, cp.STEP_DIAGONAL), k)
    h = open(os.path.join(ROOT, "mola_lidar_odometry_amd", "csrc", "mh_plan.hip")).read()
    assert "nav_tile_lw(10u, %du, nx, ny)" % (cp.TILE_X.bit_length() - 1) in h
    sw = open(os.path.join(ROOT, "mola_lidar_odometry_amd", "csrc", "mh_switches.h")).read()
    assert '"MH_PLAN_ALL_TILES"' in sw


def test_refusals_need_no_device(cp):
    L = cp.lib()
    h = C.c_void_p()
    info = cp.PlanInfo()
    one = (C.c_uint8 * 1)()
    cell = (C.c_int32 * 2)()
    price = (C.c_uint16 * 253)(*([1] * 253))
    out_len = (C.c_uint32 * 1)()
    field = (C.c_uint32 * 1)()
    assert L.mh_plan_create(None, 4, 4, C.byref(h)) == 1 and not h.value   # MH_ERR_INVALID_ARGUMENT, whatever the machine
    assert b"null" in L.mh_last_error_string()
    assert L.mh_plan_get_info(None, C.byref(info)) == 1
    assert L.mh_plan_set_cost(None, one, 0) == 1
    assert b"null" in L.mh_last_error_string()
    assert L.mh_plan_set_cost_from_nav(None, None) == 1
    assert L.mh_plan_field(None, cell, 1, 253, price, 253) == 1
    assert L.mh_plan_trace(None, cell, 1, 4, cell, out_len) == 1
    assert L.mh_plan_download(None, field) == 1
    assert L.mh_plan_destroy(None) == 0                                      # (destroying nothing is fine, as everywhere in the library)
