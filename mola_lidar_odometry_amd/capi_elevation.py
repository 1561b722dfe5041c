"""ctypes binding of include/molahip_elevation.h: the index bounds of posed key-frames, the elevation map with its two point passes,
the relief stencil and the download.  The library is capi's; this module holds the signature table of the
sixth public header and a thin handle class for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, MEM_HOST_PINNED, Context, MapFrame, _chk, _T12  # noqa: F401
from .capi_occgrid import frame_table

ELEV_API_VERSION = 1
NONE = -(1 << 31)          # MH_ELEV_NONE: the cell itself has too few points
GROUND_EMPTY = (1 << 31) - 1
TOP_EMPTY = -(1 << 31)
MAX_RELIEF_RADIUS = 4


class ElevParams(C.Structure):
    """mh_elev_params"""
    _fields_ = [("resolution", C.c_float), ("z_quantum", C.c_float), ("max_range", C.c_float), ("x0", C.c_int32), ("y0", C.c_int32),
                ("nx", C.c_uint32), ("ny", C.c_uint32), ("clearance_q", C.c_int32), ("step_q", C.c_int32), ("reserved_", C.c_uint32)]


class ElevInfo(C.Structure):
    """mh_elev_info"""
    _fields_ = [("n_offered", C.c_uint64), ("n_counted", C.c_uint64), ("n_left_out", C.c_uint64), ("n_outside_window", C.c_uint64),
                ("n_mark_offered", C.c_uint64), ("n_mark_left_out", C.c_uint64), ("n_mark_outside_window", C.c_uint64),
                ("ground_frozen", C.c_uint32), ("reserved_", C.c_uint32)]


_I32P = C.POINTER(C.c_int32)
_U32P = C.POINTER(C.c_uint32)
_FRAMES = [C.POINTER(MapFrame), C.c_size_t, C.c_int32]

_SIGNATURES = {
    "mh_elev_api_version": (C.c_uint32, []),
    "mh_elev_bounds_frames": (C.c_int32, [C.c_void_p] + _FRAMES + [C.c_float, C.c_float, C.c_uint64, _I32P, _I32P, C.POINTER(C.c_uint64)]),
    "mh_elev_create": (C.c_int32, [C.c_void_p, C.POINTER(ElevParams), C.POINTER(C.c_void_p)]),
    "mh_elev_destroy": (C.c_int32, [C.c_void_p]),
    "mh_elev_clear": (C.c_int32, [C.c_void_p]),
    "mh_elev_get_info": (C.c_int32, [C.c_void_p, C.POINTER(ElevInfo)]),
    "mh_elev_add_frames": (C.c_int32, [C.c_void_p] + _FRAMES + [C.c_uint64]),
    "mh_elev_mark_frames": (C.c_int32, [C.c_void_p] + _FRAMES + [C.c_uint64]),
    "mh_elev_relief": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, _I32P]),
    "mh_elev_download": (C.c_int32, [C.c_void_p, _I32P, _U32P, _U32P, _I32P]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_elevation.h set.  Raises if the library is absent or lacks the surface."""
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_elev_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks elevation API version {int(L.mh_elev_api_version())}, "
                          f"include/molahip_elevation.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_elevation.h")
    try:
        m = re.search(r"^#define\s+MH_ELEV_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


def ptr_table(rows):
    """MapFrame array of (x_ptr, y_ptr, z_ptr, n, T) rows: arrays the caller holds in pinned or device memory."""
    rows = list(rows)
    arr = (MapFrame * max(len(rows), 1))()
    for e, (xp, yp, zp, n, T) in zip(arr, rows):
        e.x, e.y, e.z, e.n = xp, yp, zp, int(n)
        e.T[:] = _T12(T).tolist()
    return arr, len(rows)


def _table(frames, mem):
    """(keep-alive, MapFrame array, count): (xyz [n, 3], T) pairs in host memory, or ptr_table rows for another `mem`."""
    if mem == MEM_HOST:
        keep, arr = frame_table(frames)
        return keep, arr, len(keep)
    arr, n = ptr_table(frames)
    return None, arr, n


def bounds_frames(ctx: Context, frames, resolution, max_range=0.0, max_points_per_pass=0, mem=MEM_HOST):
    """mh_elev_bounds_frames: (lo int32 [2], hi int32 [2], n_in); lo / hi are None when no point passes."""
    keep, arr, n = _table(frames, mem)
    lo, hi = np.full(2, 123456789, np.int32), np.full(2, 123456789, np.int32)
    n_in = C.c_uint64(0)
    _chk(lib().mh_elev_bounds_frames(ctx._h, arr, n, int(mem), float(resolution), float(max_range), int(max_points_per_pass),
                                     lo.ctypes.data_as(_I32P), hi.ctypes.data_as(_I32P), C.byref(n_in)))
    if n_in.value == 0:
        assert (lo == 123456789).all() and (hi == 123456789).all(), "a call without a passing point must leave lo / hi untouched"
        return None, None, 0
    return lo, hi, int(n_in.value)


class ElevMap:
    """mh_elev: a window of nx * ny cells with the planes ground, count, obstacle_count and top."""

    def __init__(self, ctx: Context, resolution=0.2, z_quantum=0.01, max_range=0.0, x0=0, y0=0, nx=1, ny=1, clearance_q=200, step_q=15):
        self.params = ElevParams(float(resolution), float(z_quantum), float(max_range), int(x0), int(y0), int(nx), int(ny),
                                 int(clearance_q), int(step_q), 0)
        self._h = C.c_void_p()
        _chk(lib().mh_elev_create(ctx._h, C.byref(self.params), C.byref(self._h)))
        self.ctx = ctx
        self.nx, self.ny = int(nx), int(ny)
        ctx._children.add(self)

    def add_frames(self, frames, max_points_per_pass=0, mem=MEM_HOST):
        keep, arr, n = _table(frames, mem)
        _chk(lib().mh_elev_add_frames(self._h, arr, n, int(mem), int(max_points_per_pass)))
        return self

    def mark_frames(self, frames, max_points_per_pass=0, mem=MEM_HOST):
        keep, arr, n = _table(frames, mem)
        _chk(lib().mh_elev_mark_frames(self._h, arr, n, int(mem), int(max_points_per_pass)))
        return self

    def clear(self):
        _chk(lib().mh_elev_clear(self._h))
        return self

    def info(self) -> ElevInfo:
        i = ElevInfo()
        _chk(lib().mh_elev_get_info(self._h, C.byref(i)))
        return i

    def relief(self, radius, min_points):
        """int32 [ny, nx]"""
        out = np.zeros((self.ny, self.nx), np.int32)
        _chk(lib().mh_elev_relief(self._h, int(radius), int(min_points), out.ctypes.data_as(_I32P)))
        return out

    def download(self):
        """(ground int32, count uint32, obstacle_count uint32, top int32), each [ny, nx]"""
        g, t = np.zeros((self.ny, self.nx), np.int32), np.zeros((self.ny, self.nx), np.int32)
        c, o = np.zeros((self.ny, self.nx), np.uint32), np.zeros((self.ny, self.nx), np.uint32)
        _chk(lib().mh_elev_download(self._h, g.ctypes.data_as(_I32P), c.ctypes.data_as(_U32P), o.ctypes.data_as(_U32P), t.ctypes.data_as(_I32P)))
        return g, c, o, t

    def close(self):
        if self._h:
            lib().mh_elev_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
