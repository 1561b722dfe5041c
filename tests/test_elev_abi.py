"""The sixth public header, include/molahip_elevation.h, the parts that need no device: what it declares is what the library exports
and what mola_lidar_odometry_amd/capi_elevation.py binds; the structures' sizes and offsets against a compiled C snippet; the
refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_elevation.h")

NAMES = ["mh_elev_add_frames", "mh_elev_api_version", "mh_elev_bounds_frames", "mh_elev_clear", "mh_elev_create", "mh_elev_destroy",
         "mh_elev_download", "mh_elev_get_info", "mh_elev_mark_frames", "mh_elev_relief"]


@pytest.fixture(scope="module")
def ce():
    from mola_lidar_odometry_amd import capi_elevation
    return capi_elevation


def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_sixth_header_is_declared_exported_and_bound(ce):
    from mola_lidar_odometry_amd import capi, capi_clean, capi_live, capi_motion, capi_occgrid
    fns = declared()
    assert fns == sorted(ce._SIGNATURES) == NAMES
    assert all(f.startswith("mh_elev_") for f in fns)
    for other in (capi, capi_clean, capi_live, capi_occgrid, capi_motion):   # nothing of it is in the other five tables
        assert not set(fns) & set(other._SIGNATURES)
    L = ce.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_elev_api_version()) == ce.ELEV_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7                                     # the first header's version is untouched
    for other, fn in ((capi_clean, "mh_clean_api_version"), (capi_live, "mh_live_api_version"), (capi_occgrid, "mh_occgrid_api_version"),
                      (capi_motion, "mh_motion_api_version")):
        assert int(getattr(other.lib(), fn)()) == 1, fn                     # ... and so are the four later ones'
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    assert {s for s in exported if s.startswith("mh_elev")} == set(fns)      # nothing of it is exported undeclared
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):               # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d
    for name in ("molahip.h", "molahip_clean.h", "molahip_live.h", "molahip_occgrid.h", "molahip_motion.h"):
        assert "mh_elev" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_the_header_compiles_as_c_and_the_layout_is_the_mirror_s(ce, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip_elevation.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mh_elev_params), offsetof(mh_elev_params, resolution), offsetof(mh_elev_params, z_quantum),
    offsetof(mh_elev_params, max_range), offsetof(mh_elev_params, x0), offsetof(mh_elev_params, y0), offsetof(mh_elev_params, nx),
    offsetof(mh_elev_params, ny), offsetof(mh_elev_params, clearance_q), offsetof(mh_elev_params, step_q));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mh_elev_info), offsetof(mh_elev_info, n_offered), offsetof(mh_elev_info, n_counted),
    offsetof(mh_elev_info, n_left_out), offsetof(mh_elev_info, n_outside_window), offsetof(mh_elev_info, n_mark_offered),
    offsetof(mh_elev_info, n_mark_left_out), offsetof(mh_elev_info, n_mark_outside_window), offsetof(mh_elev_info, ground_frozen));
  printf("%d %d %d %d %zu\n", MH_ELEV_API_VERSION, MH_ELEV_MAX_RELIEF_RADIUS, MH_ABI_VERSION, MH_ELEV_NONE == INT32_MIN, sizeof(mh_map_frame));
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b, c = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    P, I = ce.ElevParams, ce.ElevInfo
    assert [int(v) for v in a.split()] == [C.sizeof(P), P.resolution.offset, P.z_quantum.offset, P.max_range.offset, P.x0.offset, P.y0.offset,
                                           P.nx.offset, P.ny.offset, P.clearance_q.offset, P.step_q.offset] == [40, 0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert [int(v) for v in b.split()] == [C.sizeof(I), I.n_offered.offset, I.n_counted.offset, I.n_left_out.offset, I.n_outside_window.offset,
                                           I.n_mark_offered.offset, I.n_mark_left_out.offset, I.n_mark_outside_window.offset,
                                           I.ground_frozen.offset] == [64, 0, 8, 16, 24, 32, 40, 48, 56]
    assert [int(v) for v in c.split()] == [1, ce.MAX_RELIEF_RADIUS, 7, 1, C.sizeof(ce.MapFrame)] and ce.MAX_RELIEF_RADIUS == 4
    assert ce.NONE == -(1 << 31)


def test_refusals_need_no_device(ce):
    L = ce.lib()
    two = (C.c_int32 * 2)()
    n = C.c_uint64(0)
    p = ce.ElevParams(0.2, 0.01, 0.0, 0, 0, 4, 4, 200, 15, 0)
    h = C.c_void_p()
    info = ce.ElevInfo()
    arr = (ce.MapFrame * 1)()
    assert L.mh_elev_bounds_frames(None, arr, 0, 0, 0.2, 0.0, 0, two, two, C.byref(n)) == 1    # MH_ERR_INVALID_ARGUMENT, whatever the machine
    assert b"null" in L.mh_last_error_string()
    assert L.mh_elev_create(None, C.byref(p), C.byref(h)) == 1 and not h.value
    assert b"null" in L.mh_last_error_string()
    assert L.mh_elev_clear(None) == 1
    assert L.mh_elev_get_info(None, C.byref(info)) == 1
    assert L.mh_elev_add_frames(None, arr, 0, 0, 0) == 1
    assert b"null" in L.mh_last_error_string()
    assert L.mh_elev_mark_frames(None, arr, 0, 0, 0) == 1
    assert L.mh_elev_relief(None, 1, 1, two) == 1
    assert L.mh_elev_download(None, None, None, None, None) == 1
    assert L.mh_elev_destroy(None) == 0                                      # (destroying nothing is fine, as everywhere in the library)
