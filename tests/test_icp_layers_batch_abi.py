"""CPU checks of mh_icp_align_layers_batch's boundary: the declaration, the export, the binding, and the mh_layer_job layout and
MH_MAX_LAYER_BATCH_JOBS against their ctypes mirrors.  The ABI version stays 7 (a new function and a new struct are additions)."""
import ctypes as C
import os
import re
import subprocess

from mola_lidar_odometry_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")


def test_align_layers_batch_is_declared_exported_and_bound():
    assert re.search(r"MH_API\s+mh_status\s+mh_icp_align_layers_batch\s*\(", open(HEADER).read())
    assert "mh_icp_align_layers_batch" in capi._SIGNATURES
    assert hasattr(capi.lib(), "mh_icp_align_layers_batch") and callable(capi.icp_align_layers_batch)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "mola_lidar_odometry_amd", "libmolahip.so")],
                                  text=True)
    assert re.search(r"\bT mh_icp_align_layers_batch$", out, re.M)


def test_layer_job_layout_matches_c(tmp_path):
    prog = tmp_path / "lj.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip.h"
int main(void){
  printf("%zu %zu %zu %d %d %d\n", sizeof(mh_layer_job), offsetof(mh_layer_job, n_pairs), offsetof(mh_layer_job, pairs),
    MH_MAX_LAYER_BATCH_JOBS, MH_MAX_LAYER_PAIRS, MH_ABI_VERSION);
  return 0; }''')
    exe = tmp_path / "lj"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    J = capi.LayerJob
    assert vals[:3] == [C.sizeof(J), J.n_pairs.offset, J.pairs.offset]
    assert vals[3] == 64 == capi.MAX_LAYER_BATCH_JOBS
    assert vals[4] == 8 == capi.MAX_LAYER_PAIRS
    assert vals[5] == 7 == int(capi.lib().mh_abi_version())


def test_signature_takes_the_declared_arguments():
    restype, argtypes = capi._SIGNATURES["mh_icp_align_layers_batch"]
    assert restype is C.c_int32 and len(argtypes) == 8
    assert argtypes[1] is C.POINTER(capi.LayerJob) and argtypes[7] is C.POINTER(C.c_uint64)
