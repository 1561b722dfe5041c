"""CPU checks of mh_icp_align_layers_batch_opts' boundary: the declaration, the export, the binding, and the mh_layer_job_opts
layout against its ctypes mirror.  A new function and a new struct are additions: the ABI version stays 7 and mh_layer_job keeps
its layout."""
import ctypes as C
import inspect
import os
import re
import subprocess

from mola_lidar_odometry_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")
NAME = "mh_icp_align_layers_batch_opts"


def test_align_layers_batch_opts_is_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"MH_API\s+mh_status\s+%s\s*\(" % NAME, text)
    assert re.search(r"\}\s*mh_layer_job_opts\s*;", text)
    assert NAME in capi._SIGNATURES
    assert hasattr(capi.lib(), NAME) and hasattr(capi, "LayerJobOpts")
    assert "pairings_per_point" in inspect.signature(capi.icp_align_layers_batch).parameters
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "mola_lidar_odometry_amd", "libmolahip.so")],
                                  text=True)
    assert re.search(r"\bT %s$" % NAME, out, re.M)
    assert re.search(r"\bT mh_icp_align_layers_batch$", out, re.M)  # (the plain entry point stays)


def test_layer_job_opts_layout_matches_c(tmp_path):
    prog = tmp_path / "ljo.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(mh_layer_job_opts), offsetof(mh_layer_job_opts, n_pairs),
    offsetof(mh_layer_job_opts, pairs), offsetof(mh_layer_job_opts, opts), offsetof(mh_layer_job_opts, gates),
    offsetof(mh_layer_job_opts, knn), sizeof(mh_layer_job), MH_ABI_VERSION, MH_MAX_PAIRINGS_PER_POINT);
  return 0; }''')
    exe = tmp_path / "ljo"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    J = capi.LayerJobOpts
    assert vals[:6] == [C.sizeof(J), J.n_pairs.offset, J.pairs.offset, J.opts.offset, J.gates.offset, J.knn.offset]
    assert vals[6] == C.sizeof(capi.LayerJob) == C.sizeof(C.c_size_t) + C.sizeof(C.c_void_p)  # mh_layer_job is what it was
    assert vals[7] == 7 == int(capi.lib().mh_abi_version())
    assert vals[8] == 8


def test_signature_takes_the_declared_arguments():
    restype, argtypes = capi._SIGNATURES[NAME]
    plain = capi._SIGNATURES["mh_icp_align_layers_batch"][1]
    assert restype is C.c_int32 and len(argtypes) == 8
    assert argtypes[1] is C.POINTER(capi.LayerJobOpts)
    assert list(argtypes[2:]) == list(plain[2:])  # everything but the job array is mh_icp_align_layers_batch's
    assert capi.LayerJobOpts.opts.size == capi.LayerJobOpts.gates.size == capi.LayerJobOpts.knn.size == C.sizeof(C.c_void_p)
