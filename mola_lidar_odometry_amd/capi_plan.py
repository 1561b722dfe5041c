"""ctypes binding of include/molahip_plan.h: a cost plane, the cost-to-go field to the nearest of a set of goals and routes traced
down it.  The library is capi's; this module holds the signature table of the eighth public header and a thin
handle class for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, MEM_HOST_PINNED, Context, _chk  # noqa: F401

PLAN_API_VERSION = 1
UNREACHED = 0xFFFFFFFF   # MH_PLAN_UNREACHED: impassable, or not joined to a goal
TRUNCATED = 0xFFFFFFFF   # MH_PLAN_TRUNCATED: a route of more than `cap` cells
TILE_X = 64              # the relax tile, from a window at least that wide and high
TILE_Y = 16
STEP_ORTHOGONAL = 5
STEP_DIAGONAL = 7


class PlanInfo(C.Structure):
    """mh_plan_info"""
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("has_cost", C.c_uint32), ("has_field", C.c_uint32), ("passable_below", C.c_uint32),
                ("n_sweeps", C.c_uint32), ("max_field", C.c_uint32), ("reserved_", C.c_uint32), ("n_reached", C.c_uint64),
                ("n_goals_blocked", C.c_uint64), ("n_goals_outside", C.c_uint64), ("n_tile_runs", C.c_uint64)]


_U16P = C.POINTER(C.c_uint16)
_U32P = C.POINTER(C.c_uint32)
_I32P = C.POINTER(C.c_int32)

_SIGNATURES = {
    "mh_plan_api_version": (C.c_uint32, []),
    "mh_plan_create": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mh_plan_destroy": (C.c_int32, [C.c_void_p]),
    "mh_plan_get_info": (C.c_int32, [C.c_void_p, C.POINTER(PlanInfo)]),
    "mh_plan_set_cost": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mh_plan_set_cost_from_nav": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mh_plan_field": (C.c_int32, [C.c_void_p, _I32P, C.c_size_t, C.c_uint32, _U16P, C.c_size_t]),
    "mh_plan_trace": (C.c_int32, [C.c_void_p, _I32P, C.c_size_t, C.c_uint32, _I32P, _U32P]),
    "mh_plan_download": (C.c_int32, [C.c_void_p, _U32P]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_plan.h set.  Raises if the library is absent or lacks the surface."""
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_plan_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks planning API version {int(L.mh_plan_api_version())}, "
                          f"include/molahip_plan.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_plan.h")
    try:
        m = re.search(r"^#define\s+MH_PLAN_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


class PlanMap:
    """mh_plan: a window of nx * ny cells with the planes cost and field."""

    def __init__(self, ctx: Context, nx, ny):
        self._h = C.c_void_p()
        _chk(lib().mh_plan_create(ctx._h, int(nx), int(ny), C.byref(self._h)))
        self.ctx = ctx
        self.nx, self.ny = int(nx), int(ny)
        ctx._children.add(self)

    def set_cost(self, cost, mem=MEM_HOST):
        """`cost`: uint8 [ny, nx] in host memory, or an address (int) of ny * nx bytes in pinned or device memory"""
        if mem == MEM_HOST:
            cost = np.ascontiguousarray(cost, np.uint8)
            assert cost.size == self.nx * self.ny
            _chk(lib().mh_plan_set_cost(self._h, cost.ctypes.data, int(mem)))
        else:
            _chk(lib().mh_plan_set_cost(self._h, int(cost), int(mem)))
        return self

    def set_cost_from_nav(self, nav):
        """`nav`: a capi_nav.NavMap with a valid cost plane, of the same window and context"""
        _chk(lib().mh_plan_set_cost_from_nav(self._h, nav._h))
        return self

    def field(self, goals_xy, price, passable_below=253):
        """`goals_xy`: int32 [n, 2] of (column, row); `price`: uint16 [passable_below]"""
        goals = np.ascontiguousarray(goals_xy, np.int32).reshape(-1, 2)
        price = np.ascontiguousarray(price, np.uint16)
        _chk(lib().mh_plan_field(self._h, goals.ctypes.data_as(_I32P) if len(goals) else None, len(goals), int(passable_below),
                                 price.ctypes.data_as(_U16P), price.size))
        return self

    def trace(self, starts_xy, cap):
        """`starts_xy`: int32 [n, 2].  Returns (a list of int32 [len, 2] routes -- the first `cap` cells of a truncated one --, the
        uint32 [n] lengths with TRUNCATED where a route has more than `cap` cells)"""
        starts = np.ascontiguousarray(starts_xy, np.int32).reshape(-1, 2)
        n = len(starts)
        out = np.full((max(n, 1), int(cap), 2), -1, np.int32)
        lens = np.zeros(max(n, 1), np.uint32)
        _chk(lib().mh_plan_trace(self._h, starts.ctypes.data_as(_I32P) if n else None, n, int(cap), out.ctypes.data_as(_I32P),
                                 lens.ctypes.data_as(_U32P)))
        lens = lens[:n]
        return [out[i, :int(cap) if lens[i] == TRUNCATED else int(lens[i])].copy() for i in range(n)], lens

    def info(self) -> PlanInfo:
        i = PlanInfo()
        _chk(lib().mh_plan_get_info(self._h, C.byref(i)))
        return i

    def download(self):
        """the field, uint32 [ny, nx]"""
        f = np.zeros((self.ny, self.nx), np.uint32)
        _chk(lib().mh_plan_download(self._h, f.ctypes.data_as(_U32P)))
        return f

    def close(self):
        if self._h:
            lib().mh_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
