"""The size rule that lets the plan / scan matcher form the byte offsets of its gathers in 32 bits (flat_off32_sizes,
mola_lidar_odometry_amd/csrc/mh_flat_off32.h), at its boundary.  Pure arithmetic: a stand-alone C++ program compiled against the
header alone, no device.

The rule rests on "the largest index is below the element count, so the largest byte offset is at most bytes - sizeof(T)": an
allocation of exactly 2^32 bytes (a scan of exactly 2^28 points, 16 bytes each in pair_q) still passes, one element more does not."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mola_lidar_odometry_amd", "csrc")

LIM = 1 << 32        # bytes
PTS = 1 << 28        # scan points: 16 bytes each
ARGS = ("slots_bytes", "pts_bytes", "pts_q_bytes", "scan_points")
AT = {"slots_bytes": LIM, "pts_bytes": LIM, "pts_q_bytes": LIM, "scan_points": PTS}
ABOVE = {"slots_bytes": LIM + 16, "pts_bytes": LIM + 16, "pts_q_bytes": LIM + 16, "scan_points": PTS + 1}


def case(**kw):
    return tuple(kw.get(a, 0) for a in ARGS)


CASES = {"all zero": (case(), True),
         "all four at the limit": (case(**AT), True),
         "n = 2^32 - 1 does not wrap": (case(scan_points=(1 << 32) - 1), False),
         # (times 16 these are 0 and 16 modulo 2^64 -- a product would pass them -- and 2^32 modulo 2^36)
         "n = 2^60 does not wrap": (case(scan_points=1 << 60), False),
         "n = 2^60 + 1 does not wrap": (case(scan_points=(1 << 60) + 1), False),
         "n = 2^32 does not wrap": (case(scan_points=1 << 32), False)}
for a in ARGS:
    CASES["%s at the limit" % a] = (case(**{a: AT[a]}), True)
    CASES["%s one element above" % a] = (case(**{a: ABOVE[a]}), False)
    CASES["%s one element above, the others at the limit" % a] = (case(**dict(AT, **{a: ABOVE[a]})), False)
    CASES["%s one element below" % a] = (case(**{a: AT[a] - (1 if a == "scan_points" else 16)}), True)


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    d = tmp_path_factory.mktemp("flat_off32")
    rows = ",\n".join("{%dull, %dull, %dull, %dull}" % c for c, _ in CASES.values())
    prog = d / "rule.cpp"
    prog.write_text(r'''
#include <stdio.h>
#include "mh_flat_off32.h"
int main() {
  static const unsigned long long c[][4] = {
%s
  };
  for (unsigned i = 0; i < sizeof(c) / sizeof(c[0]); i++) printf("%%d\n", mh::flat_off32_sizes(c[i][0], c[i][1], c[i][2], c[i][3]) ? 1 : 0);
  return 0;
}''' % rows)
    exe = d / "rule"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(prog), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert len(out) == len(CASES)
    return dict(zip(CASES, (v == "1" for v in out)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_size_rule(verdicts, name):
    assert verdicts[name] == CASES[name][1], (name, CASES[name][0])


def test_the_header_stands_alone_and_the_launch_code_uses_it():
    """no HIP header in the rule's file (the program above compiles with g++ alone); flat_off32 is this function of the map's three
    allocations and the scan's length, nothing else"""
    src = open(os.path.join(CSRC, "mh_flat_off32.h")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ["<stddef.h>", "<stdint.h>"], includes
    launch = open(os.path.join(CSRC, "mh_k_launch.h")).read()
    assert "return mh::flat_off32_sizes(map->slots.bytes, map->pts.bytes, map->pts_q.bytes, n);" in launch
