"""ctypes binding of include/molahip_motion.h: de-skew a scan with a piecewise motion table -- K segments of constant angular
rate cut from the gyroscope samples of the sweep, one linear velocity.  The library is capi's; this module
holds the signature table of the fifth public header and thin wrappers around capi.Scan for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi
from .capi import Scan, _chk

MOTION_API_VERSION = 1
MAX_SEGMENTS = 64  # MH_MOTION_MAX_SEGMENTS


class MotionSegment(C.Structure):
    """mh_motion_segment: the start of the segment [s], the rotation there (row-major), the segment's angular rate [rad/s]."""
    _fields_ = [("knot", C.c_double), ("R", C.c_double * 9), ("w", C.c_double * 3)]


class MotionTable(C.Structure):
    """mh_motion_table: the segments (HOST memory) and the linear velocity of the whole sweep."""
    _fields_ = [("n_segments", C.c_uint32), ("reserved_", C.c_uint32), ("segments", C.POINTER(MotionSegment)),
                ("v", C.c_double * 3)]


_FP = C.POINTER(C.c_float)

_SIGNATURES = {
    "mh_motion_api_version": (C.c_uint32, []),
    "mh_scan_deskew_motion": (C.c_int32, [C.c_void_p, C.POINTER(MotionTable), C.c_void_p]),
    "mh_scan_deskew_motion_pair": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(MotionTable), C.c_void_p, C.c_void_p, _FP, _FP,
                                               C.POINTER(C.c_uint64)]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_motion.h set.  Raises if the library is absent or lacks the surface."""
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_motion_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks motion API version {int(L.mh_motion_api_version())}, "
                          f"include/molahip_motion.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_motion.h")
    try:
        m = re.search(r"^#define\s+MH_MOTION_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


def motion_table(knots, R, w, v, n_segments=None):
    """(keep-alive, MotionTable) of knots [K], R [K, 3, 3], w [K, 3], v [3]; nothing is checked here, so that a test can hand the
    library a table it must refuse.  n_segments overrides the count the structure announces."""
    knots = np.asarray(knots, np.float64).reshape(-1)
    K = len(knots)
    R = np.asarray(R, np.float64).reshape(K, 9)
    w = np.asarray(w, np.float64).reshape(K, 3)
    segs = (MotionSegment * max(K, 1))()
    for k in range(K):
        segs[k].knot = float(knots[k])
        segs[k].R[:] = R[k].tolist()
        segs[k].w[:] = w[k].tolist()
    tab = MotionTable()
    tab.n_segments = K if n_segments is None else int(n_segments)
    tab.segments = C.cast(segs, C.POINTER(MotionSegment))
    tab.v[:] = np.asarray(v, np.float64).reshape(3).tolist()
    return segs, tab


def deskew_motion(scan: Scan, table, out: Scan):
    """mh_scan_deskew_motion: `table` is None (copy) or a MotionTable; returns `out`."""
    _chk(lib().mh_scan_deskew_motion(scan._h, C.byref(table) if table is not None else None, out._h))
    return out


def deskew_motion_pair(big: Scan, small: Scan, table, out: Scan, out_small: Scan):
    """mh_scan_deskew_motion_pair: returns (bb_min, bb_max, n_finite) of the de-skewed small layer."""
    mn, mx, nf = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_uint64(0)
    _chk(lib().mh_scan_deskew_motion_pair(big._h, small._h, C.byref(table) if table is not None else None, out._h, out_small._h,
                                          mn.ctypes.data_as(_FP), mx.ctypes.data_as(_FP), C.byref(nf)))
    return mn, mx, int(nf.value)
