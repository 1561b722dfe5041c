"""CPU checks of mh_icp_align_layers' boundary: the mh_layer_pair layout against its ctypes mirror, MH_MAX_LAYER_PAIRS, and
the ABI version the header and the library speak."""
import ctypes as C
import os
import re
import subprocess

from mola_lidar_odometry_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")


def test_layer_pair_layout_matches_c(tmp_path):
    prog = tmp_path / "lp.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(mh_layer_pair), offsetof(mh_layer_pair, map), offsetof(mh_layer_pair, scan),
    offsetof(mh_layer_pair, threshold), offsetof(mh_layer_pair, threshold_angular_deg), offsetof(mh_layer_pair, weight),
    MH_MAX_LAYER_PAIRS);
  return 0; }''')
    exe = tmp_path / "lp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    L = capi.LayerPair
    assert vals[:6] == [C.sizeof(L), L.map.offset, L.scan.offset, L.threshold.offset, L.threshold_angular_deg.offset,
                        L.weight.offset]
    assert vals[6] == 8


def test_header_and_library_abi_versions_agree():
    want = int(re.search(r"^#define\s+MH_ABI_VERSION\s+(\d+)", open(HEADER).read(), re.M).group(1))
    assert want == 7
    assert int(capi.lib().mh_abi_version()) == want


def test_align_layers_is_declared_and_bound():
    assert re.search(r"MH_API\s+mh_status\s+mh_icp_align_layers\s*\(", open(HEADER).read())
    assert "mh_icp_align_layers" in capi._SIGNATURES
    assert hasattr(capi.lib(), "mh_icp_align_layers") and callable(capi.icp_align_layers)
