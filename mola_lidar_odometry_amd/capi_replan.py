"""ctypes binding of include/molahip_replan.h: repairing the cost-to-go field of an mh_plan after the cost of a rectangle of cells
changed.  The library is capi's and the handle is capi_plan's PlanMap; this module holds the signature table of the
ninth public header and three functions on a PlanMap for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, MEM_HOST_PINNED, _chk  # noqa: F401

REPLAN_API_VERSION = 1


class ReplanInfo(C.Structure):
    """mh_replan_info"""
    _fields_ = [("n_cells_changed", C.c_uint64), ("n_cells_repriced", C.c_uint64), ("n_withdrawn", C.c_uint64),
                ("n_tile_runs_withdraw", C.c_uint64), ("n_tile_runs_relax", C.c_uint64), ("n_withdraw_sweeps", C.c_uint32),
                ("n_relax_sweeps", C.c_uint32), ("n_updates", C.c_uint64), ("reserved_", C.c_uint64)]


_SIGNATURES = {
    "mh_replan_api_version": (C.c_uint32, []),
    "mh_replan_update_cost": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32]),
    "mh_replan_update_cost_from_nav": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mh_replan_get_info": (C.c_int32, [C.c_void_p, C.POINTER(ReplanInfo)]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_replan.h set.  Raises if the library is absent or lacks the surface."""
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_replan_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks replanning API version {int(L.mh_replan_api_version())}, "
                          f"include/molahip_replan.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_replan.h")
    try:
        m = re.search(r"^#define\s+MH_REPLAN_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


def update_cost(plan, x0, y0, bytes_, mem=MEM_HOST, w=None, h=None):
    """`plan`: a capi_plan.PlanMap.  `bytes_`: uint8 [h, w] in host memory, or an address (int) of h * w bytes in pinned or device
    memory together with w and h"""
    if mem == MEM_HOST:
        b = np.ascontiguousarray(bytes_, np.uint8)
        assert b.ndim == 2
        h, w = b.shape
        _chk(lib().mh_replan_update_cost(plan._h, int(x0), int(y0), int(w), int(h), b.ctypes.data, int(mem)))
    else:
        _chk(lib().mh_replan_update_cost(plan._h, int(x0), int(y0), int(w), int(h), int(bytes_), int(mem)))
    return plan


def update_cost_from_nav(plan, nav, x0, y0, w, h):
    """`nav`: a capi_nav.NavMap with a valid cost plane, of the same window and context"""
    _chk(lib().mh_replan_update_cost_from_nav(plan._h, nav._h, int(x0), int(y0), int(w), int(h)))
    return plan


def info(plan) -> ReplanInfo:
    i = ReplanInfo()
    _chk(lib().mh_replan_get_info(plan._h, C.byref(i)))
    return i
