"""ctypes binding of include/molahip_nav.h: a base cost plane, the exact squared distance to the nearest obstacle, the inflated cost
and the region reachable from seeds.  The library is capi's; this module holds the signature table of the
seventh public header and a thin handle class for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, MEM_HOST_PINNED, Context, _chk  # noqa: F401

NAV_API_VERSION = 1
FAR = 65535            # MH_NAV_FAR: no obstacle within max_cells
MAX_CELLS = 255
MAX_TABLE = 253
UNKNOWN = 255
LETHAL = 254
ROW_SEGMENT = 256      # the row pass's segment, from a window at least that wide
COL_TILE = 64          # the column pass's tile (both ways), from a window at least that wide and high
REACH_TILE_X = 64
REACH_TILE_Y = 16


class NavInfo(C.Structure):
    """mh_nav_info"""
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("has_base", C.c_uint32), ("has_cost", C.c_uint32), ("has_reach", C.c_uint32),
                ("max_cells", C.c_uint32), ("n_sweeps", C.c_uint32), ("reserved_", C.c_uint32), ("n_reached", C.c_uint64),
                ("n_seeds_blocked", C.c_uint64), ("n_seeds_outside", C.c_uint64)]


_U8P = C.POINTER(C.c_uint8)
_U16P = C.POINTER(C.c_uint16)
_I32P = C.POINTER(C.c_int32)

_SIGNATURES = {
    "mh_nav_api_version": (C.c_uint32, []),
    "mh_nav_create": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mh_nav_destroy": (C.c_int32, [C.c_void_p]),
    "mh_nav_get_info": (C.c_int32, [C.c_void_p, C.POINTER(NavInfo)]),
    "mh_nav_set_base": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mh_nav_inflate": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_int32, _U8P, C.c_size_t]),
    "mh_nav_reach": (C.c_int32, [C.c_void_p, _I32P, C.c_size_t, C.c_uint32]),
    "mh_nav_download": (C.c_int32, [C.c_void_p, _U16P, _U8P, _U8P]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_nav.h set.  Raises if the library is absent or lacks the surface."""
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_nav_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks navigation API version {int(L.mh_nav_api_version())}, "
                          f"include/molahip_nav.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_nav.h")
    try:
        m = re.search(r"^#define\s+MH_NAV_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


class NavMap:
    """mh_nav: a window of nx * ny cells with the planes base, d2, cost and reach."""

    def __init__(self, ctx: Context, nx, ny):
        self._h = C.c_void_p()
        _chk(lib().mh_nav_create(ctx._h, int(nx), int(ny), C.byref(self._h)))
        self.ctx = ctx
        self.nx, self.ny = int(nx), int(ny)
        ctx._children.add(self)

    def set_base(self, base, mem=MEM_HOST):
        """`base`: uint8 [ny, nx] in host memory, or an address (int) of ny * nx bytes in pinned or device memory"""
        if mem == MEM_HOST:
            base = np.ascontiguousarray(base, np.uint8)
            assert base.size == self.nx * self.ny
            _chk(lib().mh_nav_set_base(self._h, base.ctypes.data, int(mem)))
        else:
            _chk(lib().mh_nav_set_base(self._h, int(base), int(mem)))
        return self

    def inflate(self, max_cells, table, unknown_is_obstacle=False):
        table = np.ascontiguousarray(table, np.uint8)
        _chk(lib().mh_nav_inflate(self._h, int(max_cells), int(bool(unknown_is_obstacle)), table.ctypes.data_as(_U8P), table.size))
        return self

    def reach(self, seeds_xy, passable_below=253):
        """`seeds_xy`: int32 [n, 2] of (column, row)"""
        seeds = np.ascontiguousarray(seeds_xy, np.int32).reshape(-1, 2)
        _chk(lib().mh_nav_reach(self._h, seeds.ctypes.data_as(_I32P) if len(seeds) else None, len(seeds), int(passable_below)))
        return self

    def info(self) -> NavInfo:
        i = NavInfo()
        _chk(lib().mh_nav_get_info(self._h, C.byref(i)))
        return i

    def download(self, d2=True, cost=True, reach=True):
        """(d2 uint16, cost uint8, reach uint8), each [ny, nx]; None for a plane not asked for"""
        a = np.zeros((self.ny, self.nx), np.uint16) if d2 else None
        b = np.zeros((self.ny, self.nx), np.uint8) if cost else None
        c = np.zeros((self.ny, self.nx), np.uint8) if reach else None
        _chk(lib().mh_nav_download(self._h, a.ctypes.data_as(_U16P) if d2 else None, b.ctypes.data_as(_U8P) if cost else None,
                                   c.ctypes.data_as(_U8P) if reach else None))
        return a, b, c

    def close(self):
        if self._h:
            lib().mh_nav_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
