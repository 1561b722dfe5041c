"""ctypes binding of include/molahip_occgrid.h: key-frames ray-traced into an occupancy map at once, the index bounds of its
cells and their projection to a 2-D grid.  The library is capi's; this module holds the signature table of
the fourth public header and thin wrappers around a capi.OccMap for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, MapFrame, OccMap, _chk, _soa, _T12, _vp

OCCGRID_API_VERSION = 1
NONE = -(1 << 31)  # MH_OCCGRID_NONE: the band of this column holds no stored cell
MAX_INSERT_FRAMES = 1048576


class GridWindow(C.Structure):
    """mh_occgrid_window: the cell index of column 0 / row 0, columns and rows, the inclusive cell indices of the height band."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("nx", C.c_uint32), ("ny", C.c_uint32), ("z_lo", C.c_int32),
                ("z_hi", C.c_int32)]


_I32P = C.POINTER(C.c_int32)

_SIGNATURES = {
    "mh_occgrid_api_version": (C.c_uint32, []),
    "mh_occmap_insert_frames": (C.c_int32, [C.c_void_p, C.POINTER(MapFrame), C.c_size_t, C.c_int32, C.c_uint64]),
    "mh_occmap_index_bounds": (C.c_int32, [C.c_void_p, _I32P, _I32P, C.POINTER(C.c_uint64)]),
    "mh_occmap_project_grid": (C.c_int32, [C.c_void_p, C.POINTER(GridWindow), _I32P]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_occgrid.h set.  Raises if the library is absent or lacks the surface."""
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_occgrid_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks occupancy-grid API version {int(L.mh_occgrid_api_version())}, "
                          f"include/molahip_occgrid.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_occgrid.h")
    try:
        m = re.search(r"^#define\s+MH_OCCGRID_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


def frame_table(frames):
    """(keep-alive list, MapFrame array) of a sequence of (xyz [n, 3], T) in host memory."""
    keep = [(_soa(xyz), _T12(T)) for xyz, T in frames]
    arr = (MapFrame * max(len(keep), 1))()
    for e, ((x, y, z), T) in zip(arr, keep):
        e.x, e.y, e.z, e.n = _vp(x), _vp(y), _vp(z), len(x)
        e.T[:] = T.tolist()
    return keep, arr


def insert_frames(occ: OccMap, frames, max_points_per_pass=0, mem=MEM_HOST):
    """mh_occmap_insert_frames: `frames` is a sequence of (xyz [n, 3], T); bit for bit occ.insert() of every frame in order."""
    keep, arr = frame_table(frames)
    _chk(lib().mh_occmap_insert_frames(occ._h, arr, len(keep), int(mem), int(max_points_per_pass)))
    return occ


def insert_frames_ptr(occ: OccMap, frames, mem, max_points_per_pass=0):
    """The same from arrays the caller holds in `mem` (pinned or device): a sequence of (x_ptr, y_ptr, z_ptr, n, T)."""
    frames = list(frames)
    arr = (MapFrame * max(len(frames), 1))()
    for e, (xp, yp, zp, n, T) in zip(arr, frames):
        e.x, e.y, e.z, e.n = xp, yp, zp, int(n)
        e.T[:] = _T12(T).tolist()
    _chk(lib().mh_occmap_insert_frames(occ._h, arr, len(frames), int(mem), int(max_points_per_pass)))
    return occ


def index_bounds(occ: OccMap):
    """mh_occmap_index_bounds: (lo int32 [3], hi int32 [3], n_cells); lo / hi are None on an empty map."""
    lo, hi = np.full(3, 123456789, np.int32), np.full(3, 123456789, np.int32)
    n = C.c_uint64(0)
    _chk(lib().mh_occmap_index_bounds(occ._h, lo.ctypes.data_as(_I32P), hi.ctypes.data_as(_I32P), C.byref(n)))
    if n.value == 0:
        assert (lo == 123456789).all() and (hi == 123456789).all(), "an empty map must leave lo / hi untouched"
        return None, None, 0
    return lo, hi, int(n.value)


def project_grid(occ: OccMap, x0, y0, nx, ny, z_lo, z_hi):
    """mh_occmap_project_grid: int32 [ny, nx], the maximum log-odds per column inside the band, NONE where nothing is stored."""
    w = GridWindow(int(x0), int(y0), int(nx), int(ny), int(z_lo), int(z_hi))
    out = np.zeros((max(int(ny), 1), max(int(nx), 1)), np.int32)
    _chk(lib().mh_occmap_project_grid(occ._h, C.byref(w), out.ctypes.data_as(_I32P)))
    return out
