"""The fifth public header, include/molahip_motion.h, the parts that need no device: what it declares is what the library exports and
what mola_lidar_odometry_amd/capi_motion.py binds; the structures' sizes and offsets against a compiled C snippet; the refusals
that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_motion.h")


@pytest.fixture(scope="module")
def cm():
    from mola_lidar_odometry_amd import capi_motion
    return capi_motion


def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_fifth_header_is_declared_exported_and_bound(cm):
    from mola_lidar_odometry_amd import capi, capi_clean, capi_live, capi_occgrid
    fns = declared()
    assert fns == sorted(cm._SIGNATURES) == ["mh_motion_api_version", "mh_scan_deskew_motion", "mh_scan_deskew_motion_pair"]
    for other in (capi, capi_clean, capi_live, capi_occgrid):        # nothing of it went into another header's table
        assert not set(fns) & set(other._SIGNATURES)
    L = cm.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_motion_api_version()) == cm.MOTION_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7                              # the first header's version is untouched
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):       # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d
    first = open(os.path.join(ROOT, "include", "molahip.h")).read()
    assert "mh_motion" not in first and "mh_scan_deskew_motion" not in first


def test_the_header_compiles_as_c_and_the_layout_is_the_mirror_s(cm, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip_motion.h"
int main(void){
  printf("%zu %zu %zu %zu\n", sizeof(mh_motion_segment), offsetof(mh_motion_segment, knot), offsetof(mh_motion_segment, R), offsetof(mh_motion_segment, w));
  printf("%zu %zu %zu %zu %zu\n", sizeof(mh_motion_table), offsetof(mh_motion_table, n_segments), offsetof(mh_motion_table, reserved_),
    offsetof(mh_motion_table, segments), offsetof(mh_motion_table, v));
  printf("%d %d %d\n", MH_MOTION_API_VERSION, MH_MOTION_MAX_SEGMENTS, MH_ABI_VERSION);
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b, c = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    S, T = cm.MotionSegment, cm.MotionTable
    assert [int(v) for v in a.split()] == [C.sizeof(S), S.knot.offset, S.R.offset, S.w.offset] == [104, 0, 8, 80]
    assert [int(v) for v in b.split()] == [C.sizeof(T), T.n_segments.offset, T.reserved_.offset, T.segments.offset, T.v.offset] == [40, 0, 4, 8, 16]
    assert [int(v) for v in c.split()] == [1, cm.MAX_SEGMENTS, 7] and cm.MAX_SEGMENTS == 64


def test_refusals_need_no_device(cm):
    L = cm.lib()
    keep, tab = cm.motion_table([0.0], np.eye(3)[None], np.zeros((1, 3)), np.zeros(3))
    three = (C.c_float * 3)()
    n = C.c_uint64(0)
    assert L.mh_scan_deskew_motion(None, C.byref(tab), None) == 1               # MH_ERR_INVALID_ARGUMENT, whatever the machine
    assert b"null" in L.mh_last_error_string()
    assert L.mh_scan_deskew_motion(None, None, None) == 1
    assert L.mh_scan_deskew_motion_pair(None, None, C.byref(tab), None, None, three, three, C.byref(n)) == 1
    assert b"null" in L.mh_last_error_string()
