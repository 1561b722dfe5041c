"""The ninth public header, include/molahip_replan.h, the parts that need no device: what it declares is what the library exports and
what mola_lidar_odometry_amd/capi_replan.py binds; the structure's size and offsets against a compiled C snippet; the eight older
headers' versions and the eighth's nine exports; the switch; the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_replan.h")

NAMES = ["mh_replan_api_version", "mh_replan_get_info", "mh_replan_update_cost", "mh_replan_update_cost_from_nav"]
OLDER = ("molahip.h", "molahip_clean.h", "molahip_live.h", "molahip_occgrid.h", "molahip_motion.h", "molahip_elevation.h", "molahip_nav.h",
         "molahip_plan.h")
FIELDS = ["n_cells_changed", "n_cells_repriced", "n_withdrawn", "n_tile_runs_withdraw", "n_tile_runs_relax", "n_withdraw_sweeps", "n_relax_sweeps",
          "n_updates", "reserved_"]


@pytest.fixture(scope="module")
def cr():
    from mola_lidar_odometry_amd import capi_replan
    return capi_replan


def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_ninth_header_is_declared_exported_and_bound(cr):
    from mola_lidar_odometry_amd import capi, capi_clean, capi_elevation, capi_live, capi_motion, capi_nav, capi_occgrid, capi_plan
    fns = declared()
    assert fns == sorted(cr._SIGNATURES) == NAMES
    assert all(f.startswith("mh_replan_") for f in fns)
    for other in (capi, capi_clean, capi_live, capi_occgrid, capi_motion, capi_elevation, capi_nav, capi_plan):
        assert not set(fns) & set(other._SIGNATURES)
    L = cr.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_replan_api_version()) == cr.REPLAN_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7                                      # the first header's version is untouched
    for other, fn in ((capi_clean, "mh_clean_api_version"), (capi_live, "mh_live_api_version"), (capi_occgrid, "mh_occgrid_api_version"),
                      (capi_motion, "mh_motion_api_version"), (capi_elevation, "mh_elev_api_version"), (capi_nav, "mh_nav_api_version"),
                      (capi_plan, "mh_plan_api_version")):
        assert int(getattr(other.lib(), fn)()) == 1, fn                      # ... and so are the seven later ones'
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    assert {s for s in exported if s.startswith("mh_replan")} == set(fns)    # nothing of it is exported undeclared
    assert len({s for s in exported if s.startswith("mh_plan")}) == 9        # the eighth header's surface has not grown
    assert len({s for s in exported if s.startswith("mh_nav")}) == 8         # ... nor the seventh's
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):               # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d
    for name in OLDER:
        assert "mh_replan" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_the_header_compiles_as_c_and_the_layout_is_the_mirror_s(cr, tmp_path):
    from mola_lidar_odometry_amd import capi_plan
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip_replan.h"
int main(void){
  printf("%zu %zu", sizeof(mh_replan_info), sizeof(mh_plan_info));
''' + "".join('  printf(" %%zu", offsetof(mh_replan_info, %s));\n' % f for f in FIELDS) + r'''
  printf("\n%d %d %d %d\n", MH_REPLAN_API_VERSION, MH_PLAN_API_VERSION, MH_ABI_VERSION, MH_NAV_API_VERSION);
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    I = cr.ReplanInfo
    assert [f for f, _ in I._fields_] == FIELDS
    assert [int(v) for v in a.split()] == [C.sizeof(I), C.sizeof(capi_plan.PlanInfo)] + [getattr(I, f).offset for f in FIELDS] \
        == [64, 64, 0, 8, 16, 24, 32, 40, 44, 48, 56]
    assert [int(v) for v in b.split()] == [1, 1, 7, 1]


def test_the_switch_and_the_shared_handle(cr):
    csrc = os.path.join(ROOT, "mola_lidar_odometry_amd", "csrc")
    assert '"MH_REPLAN_FULL"' in open(os.path.join(csrc, "mh_switches.h")).read()
    assert "struct mh_plan {" in open(os.path.join(csrc, "mh_plan_internal.h")).read()
    assert "struct mh_plan {" not in open(os.path.join(csrc, "mh_plan.hip")).read()
    k = open(os.path.join(csrc, "mh_k_replan.h")).read()
    assert "k_replan_patch" in k and "k_replan_withdraw" in k and "asm" not in k


def test_refusals_need_no_device(cr):
    L = cr.lib()
    info = cr.ReplanInfo()
    one = (C.c_uint8 * 1)()
    assert L.mh_replan_update_cost(None, 0, 0, 1, 1, one, 0) == 1            # MH_ERR_INVALID_ARGUMENT, whatever the machine
    assert b"null" in L.mh_last_error_string()
    assert L.mh_replan_update_cost_from_nav(None, None, 0, 0, 1, 1) == 1
    assert L.mh_replan_get_info(None, C.byref(info)) == 1
