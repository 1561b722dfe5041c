"""The seventh public header, include/molahip_nav.h, the parts that need no device: what it declares is what the library exports and
what mola_lidar_odometry_amd/capi_nav.py binds; the structure's size and offsets against a compiled C snippet; the six older
headers' versions; the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_nav.h")

NAMES = ["mh_nav_api_version", "mh_nav_create", "mh_nav_destroy", "mh_nav_download", "mh_nav_get_info", "mh_nav_inflate", "mh_nav_reach",
         "mh_nav_set_base"]
OLDER = ("molahip.h", "molahip_clean.h", "molahip_live.h", "molahip_occgrid.h", "molahip_motion.h", "molahip_elevation.h")


@pytest.fixture(scope="module")
def cn():
    from mola_lidar_odometry_amd import capi_nav
    return capi_nav


def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_seventh_header_is_declared_exported_and_bound(cn):
    from mola_lidar_odometry_amd import capi, capi_clean, capi_elevation, capi_live, capi_motion, capi_occgrid
    fns = declared()
    assert fns == sorted(cn._SIGNATURES) == NAMES
    assert all(f.startswith("mh_nav_") for f in fns)
    for other in (capi, capi_clean, capi_live, capi_occgrid, capi_motion, capi_elevation):   # nothing of it is in the other six tables
        assert not set(fns) & set(other._SIGNATURES)
    L = cn.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_nav_api_version()) == cn.NAV_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7                                      # the first header's version is untouched
    for other, fn in ((capi_clean, "mh_clean_api_version"), (capi_live, "mh_live_api_version"), (capi_occgrid, "mh_occgrid_api_version"),
                      (capi_motion, "mh_motion_api_version"), (capi_elevation, "mh_elev_api_version")):
        assert int(getattr(other.lib(), fn)()) == 1, fn                      # ... and so are the five later ones'
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    assert {s for s in exported if s.startswith("mh_nav")} == set(fns)       # nothing of it is exported undeclared
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):               # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d
    for name in OLDER:
        assert "mh_nav" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_the_header_compiles_as_c_and_the_layout_is_the_mirror_s(cn, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip_nav.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mh_nav_info), offsetof(mh_nav_info, nx), offsetof(mh_nav_info, ny),
    offsetof(mh_nav_info, has_base), offsetof(mh_nav_info, has_cost), offsetof(mh_nav_info, has_reach), offsetof(mh_nav_info, max_cells),
    offsetof(mh_nav_info, n_sweeps), offsetof(mh_nav_info, n_reached), offsetof(mh_nav_info, n_seeds_blocked),
    offsetof(mh_nav_info, n_seeds_outside));
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", MH_NAV_API_VERSION, MH_NAV_FAR, MH_NAV_MAX_CELLS, MH_NAV_MAX_TABLE, MH_NAV_UNKNOWN, MH_NAV_LETHAL,
    MH_NAV_ROW_SEGMENT, MH_NAV_COL_TILE, MH_NAV_REACH_TILE_X, MH_NAV_REACH_TILE_Y, MH_ABI_VERSION);
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    I = cn.NavInfo
    assert [int(v) for v in a.split()] == [C.sizeof(I), I.nx.offset, I.ny.offset, I.has_base.offset, I.has_cost.offset, I.has_reach.offset,
                                           I.max_cells.offset, I.n_sweeps.offset, I.n_reached.offset, I.n_seeds_blocked.offset,
                                           I.n_seeds_outside.offset] == [56, 0, 4, 8, 12, 16, 20, 24, 32, 40, 48]
    assert [int(v) for v in b.split()] == [1, cn.FAR, cn.MAX_CELLS, cn.MAX_TABLE, cn.UNKNOWN, cn.LETHAL, cn.ROW_SEGMENT, cn.COL_TILE,
                                           cn.REACH_TILE_X, cn.REACH_TILE_Y, 7] == [1, 65535, 255, 253, 255, 254, 256, 64, 64, 16, 7]


def test_the_kernel_constants_are_the_header_s(cn):
    """the tile sizes the header names are the ones the kernels are built with"""
    k = open(os.path.join(ROOT, "mola_lidar_odometry_amd", "csrc", "mh_k_nav.h")).read()
    assert re.search(r"kRowCells = %du" % cn.ROW_SEGMENT, k)
    assert re.search(r"kColCells = %du, kColMaxLw = %du" % (cn.COL_TILE * cn.COL_TILE, cn.COL_TILE.bit_length() - 1), k)
    assert re.search(r"kReachCells = %du" % (cn.REACH_TILE_X * cn.REACH_TILE_Y), k)
    h = open(os.path.join(ROOT, "mola_lidar_odometry_amd", "csrc", "mh_nav.hip")).read()
    assert "nav_tile_lw(10u, %du, nx, ny)" % (cn.REACH_TILE_X.bit_length() - 1) in h


def test_refusals_need_no_device(cn):
    L = cn.lib()
    h = C.c_void_p()
    info = cn.NavInfo()
    one = (C.c_uint8 * 1)()
    seed = (C.c_int32 * 2)()
    assert L.mh_nav_create(None, 4, 4, C.byref(h)) == 1 and not h.value    # MH_ERR_INVALID_ARGUMENT, whatever the machine
    assert b"null" in L.mh_last_error_string()
    assert L.mh_nav_get_info(None, C.byref(info)) == 1
    assert L.mh_nav_set_base(None, one, 0) == 1
    assert b"null" in L.mh_last_error_string()
    assert L.mh_nav_inflate(None, 0, 0, one, 1) == 1
    assert L.mh_nav_reach(None, seed, 1, 253) == 1
    assert L.mh_nav_download(None, None, None, None) == 1
    assert L.mh_nav_destroy(None) == 0                                       # (destroying nothing is fine, as everywhere in the library)
