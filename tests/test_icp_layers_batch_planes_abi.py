"""CPU checks of mh_icp_align_layers_batch_planes' boundary: the declaration, the export, the binding, the mh_layer_job_planes
layout against its ctypes mirror, and which entry point capi.icp_align_layers_batch chooses.  A new function and a new struct are
additions: the ABI version stays 7 and mh_layer_job_opts keeps its layout."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")
NAME = "mh_icp_align_layers_batch_planes"


def test_align_layers_batch_planes_is_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"MH_API\s+mh_status\s+%s\s*\(" % NAME, text)
    assert re.search(r"\}\s*mh_layer_job_planes\s*;", text)
    assert "No lock-step batch form yet" not in text
    assert NAME in capi._SIGNATURES
    assert hasattr(capi.lib(), NAME) and hasattr(capi, "LayerJobPlanes")
    assert "planes_entry" in inspect.signature(capi.icp_align_layers_batch).parameters
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "mola_lidar_odometry_amd", "libmolahip.so")],
                                  text=True)
    assert re.search(r"\bT %s$" % NAME, out, re.M)
    assert re.search(r"\bT mh_icp_align_layers_batch_opts$", out, re.M)  # (the entry points before it stay)
    assert re.search(r"\bT mh_icp_align_layers_batch$", out, re.M)


def test_layer_job_planes_layout_matches_c(tmp_path):
    prog = tmp_path / "ljp.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(mh_layer_job_planes), offsetof(mh_layer_job_planes, n_pairs),
    offsetof(mh_layer_job_planes, pairs), offsetof(mh_layer_job_planes, opts), offsetof(mh_layer_job_planes, gates),
    offsetof(mh_layer_job_planes, knn), offsetof(mh_layer_job_planes, planes), sizeof(mh_layer_job_opts),
    sizeof(mh_layer_pair_plane), MH_ABI_VERSION, MH_MAX_LAYER_BATCH_JOBS);
  return 0; }''')
    exe = tmp_path / "ljp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    J = capi.LayerJobPlanes
    assert vals[:7] == [C.sizeof(J), J.n_pairs.offset, J.pairs.offset, J.opts.offset, J.gates.offset, J.knn.offset, J.planes.offset]
    assert vals[7] == C.sizeof(capi.LayerJobOpts) == C.sizeof(C.c_size_t) + 4 * C.sizeof(C.c_void_p)  # mh_layer_job_opts is what it was
    assert vals[8] == C.sizeof(capi.LayerPairPlane)
    assert vals[9] == 7 == int(capi.lib().mh_abi_version())
    assert vals[10] == capi.MAX_LAYER_BATCH_JOBS


def test_signature_takes_the_declared_arguments():
    restype, argtypes = capi._SIGNATURES[NAME]
    opts = capi._SIGNATURES["mh_icp_align_layers_batch_opts"][1]
    assert restype is C.c_int32 and len(argtypes) == 8
    assert argtypes[1] is C.POINTER(capi.LayerJobPlanes)
    assert list(argtypes[2:]) == list(opts[2:])  # everything but the job array is mh_icp_align_layers_batch_opts'
    assert capi.LayerJobPlanes.planes.size == C.sizeof(C.c_void_p)
    assert [f[0] for f in capi.LayerJobPlanes._fields_[:5]] == [f[0] for f in capi.LayerJobOpts._fields_]


class _Recorder:
    """capi.lib() with the three batch entry points replaced: they record who was called with what job type and return
    MH_ERR_INVALID_ARGUMENT, so that nothing touches a device"""

    def __init__(self):
        self.calls = []
        for name in ("mh_icp_align_layers_batch", "mh_icp_align_layers_batch_opts", NAME):
            setattr(self, name, self._make(name))

    def _make(self, name):
        def call(n, jarr, *rest):
            self.calls.append((name, type(jarr[0]).__name__, [bool(getattr(jarr[i], "planes", None)) for i in range(n)]))
            return 1
        return call

    def mh_last_error_string(self):
        return b"recorded"

    def mh_status_string(self, st):
        return b"invalid argument"


class _Handle:
    """stands in for a capi.Map / capi.Scan: _layer_pairs only reads the handle"""

    def __init__(self, n=0):
        self._h, self.n = None, n


@pytest.mark.parametrize("what, want", [("plain", "mh_icp_align_layers_batch"), ("unique", "mh_icp_align_layers_batch_opts"),
                                        ("kpp", "mh_icp_align_layers_batch_opts"), ("plane", NAME), ("forced", NAME)])
def test_capi_chooses_the_entry_point_by_the_jobs(monkeypatch, what, want):
    rec = _Recorder()
    monkeypatch.setattr(capi, "lib", lambda: rec)
    pair = dict(map=_Handle(), scan=_Handle(5), threshold=1.0)
    plane = dict(knn=10, minimum_plane_points=6, plane_eigen_threshold=1e-2, search_radius=0.8)
    jobs = [[dict(pair), dict(pair)], [dict(pair)]]
    kw = {}
    if what == "unique":
        jobs[1][0]["unique_global"] = 1
    elif what == "kpp":
        kw["pairings_per_point"] = [None, 2]
    elif what == "plane":
        jobs[0][1]["plane"] = plane
    elif what == "forced":
        kw["planes_entry"] = True
    p = capi.ICPParams(max_iterations=3, kernel_param=0.5, threshold=1.0)
    with pytest.raises(capi.MolahipError):
        capi.icp_align_layers_batch(jobs, [np.eye(4)[:3].reshape(-1)] * 2, p, **kw)
    assert len(rec.calls) == 1
    name, jtype, has_planes = rec.calls[0]
    assert name == want
    assert jtype == {"mh_icp_align_layers_batch": "LayerJob", "mh_icp_align_layers_batch_opts": "LayerJobOpts", NAME: "LayerJobPlanes"}[want]
    # only the job with a plane pair carries an array; a job without one passes NULL
    assert has_planes == ([True, False] if what == "plane" else [False, False])


def test_the_spread_jobs_end_at_four_different_iterations_on_the_reference(oracle, small_workload):
    """the four plane jobs of the GPU file's test 3, on the float64 reference alone: NoPairings after the threshold drop, nothing
    active in iteration 0, the budget with the stall test off, a stall in between"""
    import planes_batch_cases as pb
    import planes_ref as pr
    inp = pr.Inputs(small_workload)
    defs, om = pb.case_defs(inp), inp.omaps()
    assert all(pb.has_plane(defs[n]) for n in pb.SPREAD)
    refs = [pr.case_reference(defs[n], om) for n in pb.SPREAD]
    assert not any(pr.set_apart(o) for o in refs)
    names = [capi.TERM_NAMES[o["termination_reason"]] for o in refs]
    its = [o["n_iterations"] for o in refs]
    assert names == ["NoPairings", "NoPairings", "MaxIterations", "Stalled"], names
    assert its[0] == 3 and its[1] == 0 and its[2] == defs["to_the_end"]["max_it"] and 3 < its[3] < 40, its
    assert len(set(its)) == 4, its
    assert refs[2]["n_final_pairs_pt2pl"] > 0 and refs[3]["n_final_pairs_pt2pl"] > 0
